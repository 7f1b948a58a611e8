"""The consumer point code (godotoceanwaves_amd/csrc/ow_surface.h and the headers on it) where the other suites do not take it: map scales
whose two tile lengths differ, taps on the seams of a tile, the solver's Jacobian itself, and points far from the origin up to the end
of the FP32 range.  CPU builds of the headers (tests/*/ *_harness.cpp, g++ -ffp-contract=off) against the oracle bit for bit, against the
FP64 twins, and under the undefined-behaviour sanitizer.  Inputs: tests/consumer_edges.py; the device side: tests/test_consumer_edges_gpu.py;
measured margins and the mutations each test catches: profiles/consumer_edge_margins.txt."""
import os
import subprocess
import sys

import numpy as np
import pytest

import consumer as K
import consumer_edges as E
import query_twin as T
import raycast_twin as RT
from godotoceanwaves_amd import WaveGenerator as W
from oracle import oracle as O
import render_twin as RD
from checks import buoyancy_twin, check_against_twin, check_composite, check_records, compare_with_twin, fp32_slack, SHADE_TOL
from consumer_edges import far_bodies, float_fields_finite, OPTION_SETS, seam_camera
from cpu_builds import cpu_buoyancy, cpu_query, cpu_query_velocity, cpu_raycast, cpu_render, cpu_sample, CpuSet, CSRC, HERE
from cpu_builds import bodies_harness, buoyancy_harness, query_harness, raycast_harness, render_harness, velocity_harness  # noqa: F401 (fixtures)
from scenes import (bilinear64, blob_hull, camera_rays, demo_scene, G, make_bodies, maps_u16, pixel_rays, quaternion, query_points,
                    ray_options, RAY_TOL as TOL, RHO, sampling_case, slope_factor, SPACING, SUN_LOW, unit)

REC = W.SURFACE_QUERY


# ---- the seam points reach what they are built for ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [128, 256, 1024, 2048])
def test_seam_points_hit_every_class_in_every_cascade(query_harness, n):
    """per cascade: taps with c0 = n - 1 alone, r0 = n - 1 alone and both, in the tile at the origin and one and seven tiles away on the
    negative side; exact texel centres (weight 0) and edges (weight 0.5); and make_tap's integers are the NumPy ones"""
    xz = E.seam_points(E.EDGE_SCALES, n)
    c0, r0 = E.tap_integers(E.EDGE_SCALES, n, xz)
    for i, (sx, sy, _, _) in enumerate(E.EDGE_SCALES):
        uv = np.ascontiguousarray(np.stack([xz[:, 0] * sx, xz[:, 1] * sy], axis=1), np.float32)
        taps = np.zeros((len(uv), 4), np.int32)
        w = np.zeros((len(uv), 2), np.float32)
        query_harness.harness_tap(uv.ctypes.data, len(uv), n, taps.ctypes.data, w.ctypes.data)
        assert np.array_equal(taps[:, 2], c0[i]) and np.array_equal(taps[:, 0], r0[i])
        assert np.array_equal(taps[:, 3], (c0[i] + 1) % n) and np.array_equal(taps[:, 1], (r0[i] + 1) % n)
        last_c, last_r = c0[i] == n - 1, r0[i] == n - 1
        tile = np.floor(xz.astype(np.float64) * [sx, sy] + 0.5)   # the tile whose border the point sits beside
        for lo, hi in ((0, 1), (-1, -1), (-7, -7)):
            here_x, here_z = (tile[:, 0] >= lo) & (tile[:, 0] <= hi), (tile[:, 1] >= lo) & (tile[:, 1] <= hi)
            assert (last_c & ~last_r & here_x).any() and (~last_c & last_r & here_z).any() and (last_c & last_r & here_x & here_z).any(), (i, lo)
        assert (w[:, 0] == 0).any() and (w[:, 1] == 0).any() and (w[:, 0] == 0.5).any() and (w[:, 1] == 0.5).any(), i


# ---- A1. sample_point is the oracle's owo_sample_surface, bit for bit --------------------------------------------------------------------

@pytest.mark.parametrize("case", ["random_maps", "generated_maps", "spray_active", "fine_cascades", "edge_scales"])
def test_sample_point_is_the_oracles_bit_for_bit(query_harness, case):
    """the CPU build of ow_surface.h's sample_point against the oracle's restatement of the .gdshader text, every field, the spray
    decision included: the four cases tests/test_surface_sampling.py pins to the reference's shaders, and EDGE_SCALES on the pipeline's
    own maps with the seam points and the far points.  Inside the range where the old integer conversions were defined the oracle is an
    independent statement, pinned to the reference's shader text by tests/test_surface_sampling.py; beyond it (from 2^63 texels, and
    where the coordinate overflows) the reference defines nothing, and the oracle and the header hold the same rule by construction --
    there this comparison says only that the two copies of it agree, and the finiteness assertion is the check."""
    if case == "edge_scales":
        d, m, sc = E.edge_maps(128)
        far, bad = E.far_points()
        xz = np.concatenate([E.seam_points(sc, 128), far, bad, query_points(2000, seed=13)])
    else:
        d, m, sc, xz = sampling_case(case)
    got = cpu_sample(query_harness, d, m, sc, xz)
    want = O.sample_surface(np.asarray(d), np.asarray(m), sc, xz)
    for f in O.SURFACE_SAMPLE.names:
        assert got[f].tobytes() == want[f].tobytes(), f
    float_fields_finite(got)
    if case == "spray_active":
        assert 0 < got["spray_active"].sum() < len(xz)
    if case == "edge_scales":   # the non-square fragment mix: one cascade takes the bilinear lookup alone, another does not
        ppm = 128 * E.EDGE_SCALES[:, :2].min(axis=1)
        assert (ppm * 0.1 >= 1).any() and (ppm * 0.1 < 1).any()
        assert np.abs(got["gradient_fragment"] - got["gradient_scaled"]).max() > 1e-3


# ---- A2. query_eval against the analytic FP64 Jacobian -------------------------------------------------------------------------------------

# max |J32 - J64| / max |J64| and max |F32 - F64| / max |F64| measured on the CPU build over the points of jacobian_case (20 000 in
# +-400 m, 128^2 maps of edge_records, border exclusion 2^-10 texels), and asserted at four times that: profiles/consumer_edge_margins.txt
MEASURED = {None: dict(J=8.21e-5, F=4.54e-6), (250.0, -200.0): dict(J=6.41e-5, F=5.79e-6)}
BORDER = 2.0 ** -10


def jacobian_case():
    d, m, sc = E.edge_maps(128)
    rng = np.random.default_rng(17)
    p = rng.uniform(-400, 400, (20000, 2)).astype(np.float32)
    q = (p + rng.normal(0, 0.5, p.shape)).astype(np.float32)
    return d, sc, p, q


def eval_cpu(L, d, sc, p, q, center):
    pq = np.ascontiguousarray(np.concatenate([p, q], axis=1), np.float32)
    out = np.zeros((len(pq), 8), np.float32)
    d = maps_u16(d)
    s = np.ascontiguousarray(sc, np.float32)
    cx, cz = center if center is not None else (0.0, 0.0)
    L.harness_eval(d.ctypes.data, d.shape[1], len(s), s.ctypes.data, pq.ctypes.data, len(pq), int(center is not None), cx, cz, out.ctypes.data)
    return out[:, 0:2], out[:, 2:6].reshape(-1, 2, 2), out[:, 6], out[:, 7]


def jacobian_rounding_bound(d, sc, p):
    """how far an FP32 Jacobian entry may sit from the FP64 one inside the same cell: the texel coordinate p s N is rounded twice
    (|p| s N 2^-22 texels), which moves a bilinear derivative by that many texels times the cell's mixed difference (d - c) - (b - a),
    times N s |scales.z| -- summed over the cascades -- plus the rounding of the sums (a few ulp of the largest term)"""
    D = T.as_f64(d)
    sc = np.asarray(sc, np.float64)
    n = D.shape[1]
    r = np.abs(np.asarray(p, np.float64)).max()
    total, terms = 0.0, 0.0
    for i in range(len(sc)):
        L = D[i][..., [0, 2]]
        mixed = np.abs(np.roll(np.roll(L, -1, 0), -1, 1) - np.roll(L, -1, 0) - np.roll(L, -1, 1) + L).max()
        first = max(np.abs(np.diff(L, axis=a)).max() for a in (0, 1))
        k = n * sc[i, :2].max() * abs(sc[i, 2])
        total += k * mixed * r * sc[i, :2].max() * n * 2.0 ** -22
        terms += k * first
    return total + 8 * 2.0 ** -24 * terms


@pytest.mark.parametrize("center", [None, (250.0, -200.0)], ids=["no_falloff", "falloff"])
def test_query_eval_against_the_analytic_jacobian(query_harness, center):
    """F and the four entries of J as query_eval forms them, against query_twin.jacobian and query_twin.forward in FP64 at the same FP32
    p.  Without a centre, and with one most points lie more than 150 m from, so that S (x) grad f carries weight.  J jumps at cell
    borders and an FP32 coordinate can sit on the other side of one: a point within 2^-10 texels of a border -- any cascade, either axis
    -- is left out, and no more than 3 % may be (5 cascades x 2 axes x 2 sides x 2^-10 is 2 %)."""
    d, sc, p, q = jacobian_case()
    F32, J32, f32, r32 = eval_cpu(query_harness, d, sc, p, q, center)
    J64, border = T.jacobian(d, sc, p, center)
    fwd, _ = T.forward(d, sc, p, center)
    F64 = fwd - q.astype(np.float64)
    keep = border >= BORDER
    excluded = 1.0 - keep.mean()
    assert excluded <= 0.03, excluded
    if center is not None:
        dist = np.hypot(p[:, 0] - center[0], p[:, 1] - center[1])
        assert (dist > 150).mean() > 0.5
        assert np.abs(J64 - T.jacobian(d, sc, p, None)[0])[keep].max() > 0.1   # the falloff terms are not a rounding matter
    errJ = np.abs(J32 - J64)[keep].max() / np.abs(J64).max()
    errF = np.abs(F32 - F64).max() / np.abs(F64).max()
    slack = fp32_slack(d, sc, p)
    boundJ = jacobian_rounding_bound(d, sc, p)
    print(f"centre {center}: J {errJ:.3e} of max |J| {np.abs(J64).max():.3f} (rounding bound {boundJ / np.abs(J64).max():.3e}), "
          f"F {errF:.3e} of max |F| {np.abs(F64).max():.3f} (slack up to {slack.max():.3e} m), excluded {excluded:.4f}")
    assert errJ <= 4 * MEASURED[center]["J"] and errF <= 4 * MEASURED[center]["F"]
    assert (np.abs(J32 - J64)[keep].max(axis=(1, 2)) <= boundJ).all()
    assert (np.abs(F32 - F64).max(axis=1) <= slack).all()
    assert np.abs(f32 - T.falloff(p, center)).max() <= 4e-7
    assert np.abs(r32 - np.hypot(F64[:, 0], F64[:, 1])).max() <= 2 * slack.max()
    assert np.abs(np.linalg.det(J64) - 1).max() > 0.5   # a Jacobian far from the identity: the comparison is not of I with I


# ---- A3. non-square tiles through every consumer's own twin check ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [128, 256])
def test_query_on_non_square_tiles_against_the_fp64_twin(query_harness, n):
    d, m, sc = E.edge_maps(n)
    xz = np.concatenate([E.seam_points(sc, n), query_points(3000, seed=3)])
    out = cpu_query(query_harness, d, m, sc, xz)
    c = check_against_twin(out, d, sc, xz)
    assert c.mean() > 0.5
    s = cpu_sample(query_harness, d, m, sc, out["p"])
    assert out["sample"].tobytes() == s.tobytes()
    center = (40.0, -25.0)
    xz = (np.random.default_rng(4).uniform(-600, 600, (3000, 2)) + center).astype(np.float32)
    out = cpu_query(query_harness, d, m, sc, xz, falloff_center=center)
    check_against_twin(out, d, sc, xz, center=center)
    f64 = T.falloff(out["p"], center)
    assert np.abs(out["falloff"] - f64).max() <= 4e-7 * f64.max() + 1e-30
    assert np.array_equal(out["height"], out["falloff"] * out["sample"]["displacement"][:, 1])


ROUND_TRIP_SCALE = 0.25


def test_round_trip_on_a_non_square_calm_sea(query_harness):
    """cascade 3 of edge_records (250 x 137 m) at a displacement scale under which the forward map does not fold: q = forward(p0) has one
    preimage and the query has to find it.  The bounds are tests/test_surface_query.py test_round_trip_on_a_calm_sea's."""
    d, m, _ = E.edge_maps(256)
    d, m = d[3:4], m[3:4]
    sc = E.EDGE_SCALES[3:4].copy()
    sc[:, 2] = ROUND_TRIP_SCALE
    assert T.min_det_on_lattice(d, sc) > 0.25
    rng = np.random.default_rng(7)
    p0 = rng.uniform(-300, 300, (10000, 2))
    q64, h64 = T.forward(d, sc, p0)
    out = cpu_query(query_harness, d, m, sc, q64.astype(np.float32), tolerance=1e-4)
    assert (out["converged"] == 1).all()
    err = np.hypot(*(out["p"] - p0).T)
    assert err.max() <= 1e-3, err.max()
    assert np.abs(out["height"] - h64).max() <= 1e-4
    assert np.abs(q64 - p0).max() > 0.05   # the displacement the query undoes is not nothing


def test_min_det_lattice_spans_each_axis_on_its_own():
    """a fold that only a lattice over the whole z span of the tile reaches: one row of steep D_z near the far end of the longer axis"""
    n = 32
    d = np.zeros((1, n, n, 4), np.float16)
    d[0, n - 2, :, 2] = 4.0      # D_z jumps by 4 m over one texel of 64 / 32 = 2 m, near z = 60 m of a 16 x 64 m tile
    sc = np.array([(1 / 16.0, 1 / 64.0, 1.0, 1.0)], np.float32)
    assert T.min_det_on_lattice(maps_u16(d), sc) < 0


def test_buoyancy_sums_on_non_square_tiles_against_the_fp64_twin(buoyancy_harness):
    """tests/test_buoyancy.py test_per_body_sums_against_the_fp64_twin's assertion and bounds, on EDGE_SCALES at 256^2"""
    d, _, sc = E.edge_maps(256)
    bodies, hull = demo_scene()
    for opts in ({}, {"water_level": 0.4, "density": 1000.0, "gravity": 9.8}, {"falloff_center": (30.0, -60.0)}):
        res, pts = cpu_buoyancy(buoyancy_harness, d, sc, bodies, hull, opts)
        F, Tq, SV = buoyancy_twin(d, sc, bodies, hull, pts["p"], opts)
        for b, body in enumerate(bodies):
            sl = slice(body["point_offset"], body["point_offset"] + body["point_count"])
            full = opts.get("density", RHO) * opts.get("gravity", G) * hull[sl]["volume"].astype(np.float64).sum()
            arm = np.linalg.norm(hull[sl]["local"], axis=1).max()
            assert np.abs(res[b]["force"] - F[b]).max() <= 2e-5 * full, (b, res[b]["force"], F[b])
            assert np.abs(res[b]["torque"] - Tq[b]).max() <= 2e-5 * full * arm, (b, res[b]["torque"], Tq[b])
            assert abs(res[b]["submerged_volume"] - SV[b]) <= 2e-5 * hull[sl]["volume"].sum()
        assert (res["invalid_points"] == 0).all() and res["wetted_points"].sum() > 0
        assert 0 < (SV > 0).sum() and ((SV > 0) & (SV < hull["volume"].sum())).any()
        # a point's height is the twin's displacement sum at its p: ow_buoyancy.h's own one-tap-per-cascade lookup on non-square tiles
        h64 = T.displacement(d, sc, pts["p"])[:, 1] * T.falloff(pts["p"], opts.get("falloff_center"))
        assert np.abs(pts["height"] - h64).max() <= 1e-5 * np.abs(h64).max() + fp32_slack(d, sc, pts["p"]).max()


def skew_swell_maps(n=256, tile=(100.0, 60.0), amplitude=1.5, waves=(5, 4)):
    """D_xz = 0, D_y = A cos(kx x + kz z) at the texel centres of a non-square tile, kx != kz: a height-only swell that is not
    symmetric in x and z (the query's p is q)"""
    x = (np.arange(n) + 0.5) * tile[0] / n
    z = (np.arange(n) + 0.5) * tile[1] / n
    kx, kz = 2 * np.pi * waves[0] / tile[0], 2 * np.pi * waves[1] / tile[1]
    d = np.zeros((1, n, n, 4), np.float16)
    d[0, :, :, 1] = amplitude * np.cos(kx * x[None, :] + kz * z[:, None])   # rows run along z, columns along x
    return maps_u16(d), np.zeros((1, n, n, 4), np.uint16), np.array([(1 / tile[0], 1 / tile[1], -1.0, 1.0)], np.float32), amplitude * np.hypot(kx, kz)


def test_skew_swell_cast_against_the_fp64_twin(raycast_harness, query_harness):
    """tests/test_raycast.py test_swell_against_the_fp64_twin's assertions and bounds on a swell whose crests run askew over a 100 x 60 m
    tile, under a negative displacement scale (the slab takes its magnitude)"""
    d, m, sc, steepest = skew_swell_maps()
    rays = camera_rays(300, (2.0, 60.0), (3.0, 80.0), seed=11, max_distance=3000.0)
    out, mh = cpu_raycast(raycast_harness, d, m, sc, rays, probe=True)
    hit = check_records(raycast_harness, query_harness, d, m, sc, rays, out)
    assert hit.all()
    dn = unit(rays["direction"]).astype(np.float64)
    t_star = RT.raycast(RT.Field(d, sc), rays["origin"].astype(np.float64), dn, out["t_enter"].astype(np.float64),
                        out["t_exit"].astype(np.float64), SPACING / 16)
    err = np.abs(out["t"] - t_star)
    assert np.isfinite(t_star).all() and err.max() <= TOL + 1e-5, err.max()
    assert (np.abs(out["residual"]) <= TOL * slope_factor(dn, steepest) + 1e-5).all()
    assert (mh <= out["slab_half_height"]).all() and 1.5 <= out["slab_half_height"][0] <= 1.5 * (1 + 2 ** -10) + 0.01 + 1e-6


def test_velocity_query_on_non_square_tiles_against_the_fp64_twin(velocity_harness):
    """tests/test_water_velocity.py test_host_velocity_and_moving_drag_against_the_fp64_twin's velocity bound, on EDGE_SCALES: the
    displacement maps are the pipeline's, the velocity layers random (every texel differs from its neighbours in both directions)"""
    d, _, sc = E.edge_maps(128)
    rng = np.random.default_rng(2)
    vel = rng.normal(0, 2.0, d.shape).astype(np.float16)
    vel[..., 3] = 0
    xz = np.concatenate([E.seam_points(sc, 128), rng.uniform(-300, 300, (3000, 2)).astype(np.float32)])
    for center in (None, (30.0, -80.0)):
        got = cpu_query_velocity(velocity_harness, d, vel, sc, xz, center)
        assert all(np.isfinite(got[f]).all() for f in ("velocity", "height", "p"))
        p = got["p"].astype(np.float64)
        f = T.falloff(p, center)
        want = sum(bilinear64(vel[i], p[:, 0] * sc[i, 0], p[:, 1] * sc[i, 1])[:, :3] * sc[i, 2] for i in range(len(sc))) * f[:, None]
        step = sum(abs(sc[i, 2]) * max(np.abs(np.diff(vel[i][..., :3].astype(np.float64), axis=a)).max() for a in (0, 1)) for i in range(len(sc)))
        coord = np.abs(p).max() * sc[:, :2].max() * d.shape[1] * 2.0 ** -22
        err = np.abs(got["velocity"] - want)
        assert err.max() <= 1e-6 * np.abs(want).max() + coord * step, (err.max(), coord * step)
        assert np.abs(want).max() > 1.0


def height_slack(d, sc, p):
    """test_surface_query.fp32_slack for the height: the FP32 lookup of D_y at p against the FP64 one -- the texel coordinate's rounding
    (|p| s N 2^-22 texels) times each cascade's largest texel step of D_y, plus a few ulp of the position and the sum"""
    D = T.as_f64(d)
    s64 = np.asarray(sc, np.float64)
    r = np.abs(np.asarray(p, np.float64)).max(axis=-1)
    per_texel = sum(abs(s64[i, 2]) * max(np.abs(np.diff(D[i][..., 1], axis=a)).max() for a in (0, 1)) for i in range(len(s64)))
    return 2e-5 + r * 2.0 ** -21 + r * s64[:, :2].max() * D.shape[1] * 2.0 ** -22 * per_texel


def test_render_on_non_square_tiles_against_the_twins(render_harness, raycast_harness):
    """a view from above a seam over EDGE_SCALES at 256^2: the pixel rays against render_twin's, every pixel the ray cast's bits, the
    record's height the FP64 displacement sum at its p (ow_render.h's own lookups on non-square tiles), and the shading against
    render_twin.shade within tests/test_render_view.py's SHADE_TOL"""
    d, m, sc = E.edge_maps(256)
    opts = dict(roughness=0.4, normal_strength=1.0, light_direction=SUN_LOW, falloff=True)
    cam = seam_camera(sc, 256, width=24, height=16)
    rays = pixel_rays(render_harness, cam)
    want_dir = RD.pixel_directions(list(cam.basis), cam.fov_y_degrees, cam.width, cam.height).reshape(-1, 3)
    dn = rays["direction"]
    assert np.abs(dn / np.sqrt((dn[:, 0] * dn[:, 0] + dn[:, 1] * dn[:, 1]) + dn[:, 2] * dn[:, 2])[:, None] - want_dir).max() <= 1e-6
    rgba, rec = cpu_render(render_harness, d, m, sc, cam, opts)
    hit = check_composite(rgba, rec, opts)
    assert hit.mean() > 0.5
    cast = cpu_raycast(raycast_harness, d, m, sc, rays, ray_options(opts, cam)).reshape(rec.shape)
    assert np.array_equal(rec["status"], cast["status"]) and rec["t"].tobytes() == cast["t"].tobytes()
    assert rec["p"].tobytes() == cast["query"]["p"].tobytes()
    assert rec["gradient_fragment"].tobytes() == cast["query"]["sample"]["gradient_fragment"].tobytes()
    p = rec["p"][hit].astype(np.float64)
    h64 = T.displacement(d, sc, p)[:, 1]
    assert (np.abs(rec["wave_height"][hit] - h64) <= height_slack(d, sc, p)).all()
    g64 = K.gradient_fragment_at([T.as_f64(m)[i] for i in range(len(sc))], sc.astype(np.float64), p[:, 0], p[:, 1])
    assert np.abs(rec["gradient_fragment"][hit] - g64[:, :2]).max() <= 2e-4 and np.abs(rec["foam_fragment"][hit] - g64[:, 2]).max() <= 2e-4
    worst, count = compare_with_twin(rec, cam, opts)
    assert count > 100
    for k, v in worst.items():
        assert v <= SHADE_TOL, (k, v)


@pytest.mark.parametrize("opts", [{}, {"warm_start": True}], ids=["cold", "warm"])
def test_a_floating_body_on_non_square_tiles_is_the_cpu_buoyancy_at_every_pose(bodies_harness, buoyancy_harness, opts):
    """one free body of 65 hull points dropped on a seam of EDGE_SCALES at 256^2: every substep's results and point records are the
    buoyancy CPU build's at the pose the harness reports (tests/test_bodies_step.py's assertion), and each point's height is the FP64
    displacement sum at its p"""
    d, _, sc = E.edge_maps(256)
    x, z = E.seam_points(sc, 256)[2]
    size = (4.0, 1.5, 6.0)
    st, hull = make_bodies([dict(hull=blob_hull(65, size, 0, 11), size=size, origin=(float(x), 0.3, float(z)), q=quaternion((1.0, 0.2, -0.4), 0.3),
                                 v=(1.5, 0.0, -0.8), w=(0.1, 0.2, -0.1), kl=0.6, kq=0.2, density=500.0)])
    cs = CpuSet(bodies_harness, st, hull)
    pts = np.zeros(len(hull), W.BUOYANCY_POINT)
    for k in range(12):
        tr, tb = cs.step(d, sc, 1, 1.0 / 60.0, opts, trace=True)
        want, pts = cpu_buoyancy(buoyancy_harness, d, sc, tb[0], hull, opts, points=pts if opts.get("warm_start") else None)
        assert tr[0].tobytes() == want.tobytes() and cs.pts.tobytes() == pts.tobytes() and cs.results.tobytes() == want.tobytes(), k
        h64 = T.displacement(d, sc, cs.pts["p"])[:, 1]
        assert (np.abs(cs.pts["height"] - h64) <= height_slack(d, sc, cs.pts["p"])).all(), k
    assert cs.results["wetted_points"][0] > 0 and cs.results["invalid_points"][0] == 0 and (cs.flags == 0).all()
    assert np.abs(cs.state["position"] - st["position"]).max() > 0.1


# ---- A5. far points ------------------------------------------------------------------------------------------------------------------------

def test_far_points_leave_nothing_non_finite_in_a_query_record(query_harness):
    d, m, sc = E.edge_maps(128)
    far, bad = E.far_points()
    for kw in OPTION_SETS:
        out = cpu_query(query_harness, d, m, sc, far, **kw)
        float_fields_finite(out)
        assert set(np.unique(out["converged"])) <= {0, 1}
        assert out["world_xz"].tobytes() == far.tobytes()
        assert (out["iterations"] <= (kw.get("max_iterations") or 16)).all() and (out["iterations"] >= 0).all()
        near = np.abs(far).max(axis=1) <= 1e12      # inside kCoordMax tiles of every cascade: solved like any point
        assert (np.abs(out["p"][near] - far[near]) <= 16.0 + np.abs(far[near]) * 2.0 ** -22).all()
        beyond = np.abs(far).max(axis=1) >= 3e38    # beyond it: refused like a non-finite q
        assert (out["p"][beyond] == 0).all() and (out["converged"][beyond] == 0).all()
        out = cpu_query(query_harness, d, m, sc, bad, **kw)
        for f in REC.names:   # world_xz echoes the non-finite q; nothing else may hold one
            if f == "sample":
                float_fields_finite(out[f])
            elif f != "world_xz" and REC.fields[f][0].base.kind == "f":
                assert np.isfinite(out[f]).all(), f
        assert (out["p"] == 0).all() and (out["converged"] == 0).all() and (out["iterations"] == 0).all()


def test_far_points_leave_nothing_non_finite_in_buoyancy_cast_or_velocity(buoyancy_harness, raycast_harness, velocity_harness, query_harness):
    d, m, sc = E.edge_maps(128)
    far, bad = E.far_points()
    bodies, hull = far_bodies(far)
    for opts in ({}, {"falloff_center": (12.5, -40.0)}, {"warm_start": True}):
        res, pts = cpu_buoyancy(buoyancy_harness, d, sc, bodies, hull, opts)
        float_fields_finite(res)
        float_fields_finite(pts)
        assert set(np.unique(pts["converged"])) <= {0, 1}
    assert (res["invalid_points"][:8] == 0).all()   # 1e5 m is an ordinary place for a body
    # the cast: far origins looking down, and rays that start near the origin and run out to the far points
    o = np.stack([far[:, 0], np.full(len(far), 30.0, np.float32), far[:, 1]], axis=1)
    rays = np.concatenate([W.rays(o, np.tile([(0.1, -1.0, 0.2)], (len(o), 1)), 500.0),
                           W.rays(np.tile([(3.0, 20.0, -4.0)], (len(o), 1)), np.stack([far[:, 0], np.full(len(far), -1.0), far[:, 1]], axis=1), 3e38)])
    for opts in (None, {"falloff_center": (0.0, 0.0)}):
        out = cpu_raycast(raycast_harness, d, m, sc, rays, opts)
        float_fields_finite(out)
    for center in (None, (12.5, -40.0)):
        v = cpu_query_velocity(velocity_harness, d, m, sc, np.concatenate([far, bad]), center)
        float_fields_finite(v)
        assert set(np.unique(v["converged"])) <= {0, 1} and (v["converged"][len(far):] == 0).all()


# ---- the same points under the undefined-behaviour sanitizer --------------------------------------------------------------------------------

UBSAN = ["-fsanitize=undefined,float-cast-overflow"]


def ubsan_available(tmp):
    src = os.path.join(tmp, "probe.cpp")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    return subprocess.run(["g++", "-fsanitize=undefined", src, "-o", os.path.join(tmp, "probe")], capture_output=True).returncode == 0


CHILD = r"""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.dirname(sys.argv[1]))
import consumer as K
import consumer_edges as E
import cpu_builds as B
from godotoceanwaves_amd import WaveGenerator as W
def load(name):
    return C.CDLL(os.path.join(sys.argv[2], "lib%s_harness.so" % name))
d, m, sc = E.edge_maps(128)
far, bad = E.far_points()
pts = np.concatenate([E.seam_points(sc, 128), far, bad])
Vp = C.c_void_p
q = load("query")
q.harness_sample.argtypes = [Vp, Vp, C.c_int, C.c_int, Vp, Vp, C.c_int, Vp]
q.harness_query.argtypes = [Vp, Vp, C.c_int, C.c_int, Vp, Vp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float, Vp]
for kw in E.OPTION_SETS:
    B.cpu_query(q, d, m, sc, pts, **kw)
B.cpu_sample(q, d, m, sc, pts)
b = load("buoyancy")
b.harness_buoyancy.argtypes = [Vp, C.c_int, C.c_int, Vp, Vp, C.c_int, Vp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, Vp, Vp]
bodies, hull = E.far_bodies(np.concatenate([E.seam_points(sc, 128)[::7], far]))
for opts in ({}, {"falloff_center": (12.5, -40.0)}, {"warm_start": True}):
    B.cpu_buoyancy(b, d, sc, bodies, hull, opts)
r = load("raycast")
r.harness_raycast.argtypes = [Vp, Vp, C.c_int, C.c_int, Vp, Vp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, Vp, Vp]
fin = np.concatenate([E.seam_points(sc, 128)[::5], far])
o = np.stack([fin[:, 0], np.full(len(fin), 30.0, np.float32), fin[:, 1]], axis=1)
B.cpu_raycast(r, d, m, sc, W.rays(o, np.tile([(0.1, -1.0, 0.2)], (len(o), 1)), 500.0))
B.cpu_raycast(r, d, m, sc, W.rays(np.tile([(3.0, 20.0, -4.0)], (len(o), 1)), np.stack([fin[:, 0], np.full(len(fin), -1.0), fin[:, 1]], axis=1), 3e38))
v = load("velocity")
v.harness_query_velocity.argtypes = [Vp, Vp, C.c_int, C.c_int, Vp, Vp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float, Vp]
for center in (None, (12.5, -40.0)):
    B.cpu_query_velocity(v, d, m, sc, pts, center)
print("ran", len(pts), "points")
"""


def test_no_undefined_behaviour_on_far_and_seam_points(tmp_path):
    """the query, buoyancy, ray-cast and velocity harnesses built a second time with -fsanitize=undefined,float-cast-overflow, and the far
    and seam points run through them in a child process: no `runtime error` on its stderr"""
    if not ubsan_available(str(tmp_path)):
        pytest.skip("libubsan cannot be linked on this machine")
    for name in ("query", "buoyancy", "raycast", "velocity"):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas"] + UBSAN +
                       ["-I", CSRC, os.path.join(HERE, name, name + "_harness.cpp"), "-o", str(tmp_path / ("lib%s_harness.so" % name))], check=True)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=0")
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    run = subprocess.run([sys.executable, str(script), HERE, str(tmp_path)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stderr[-4000:]
    assert "ran" in run.stdout
    assert "runtime error" not in run.stderr, run.stderr[-4000:]

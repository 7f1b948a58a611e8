"""The device side of tests/test_consumer_edges.py: the consumer kernels on map scales whose two tile lengths differ, on taps that sit on
the seams of a tile (the two-8-byte-loads branch of load_quad exists on the device only), and on points out to the end of the FP32 range
and beyond.  Every record is held to the CPU build of the same header bit for bit, ow_sample_surface to the oracle; the maps are the
device's own, from tests/consumer_edges.py edge_records()."""
import ctypes as C

import numpy as np
import pytest

import consumer_edges as E
from godotoceanwaves_amd import WaveCascadeParameters, WaveGenerator as W
from godotoceanwaves_amd.presets import UPDATE_DELTA
from oracle import oracle as O
from checks import assert_same_image
from consumer_edges import float_fields_finite, OPTION_SETS, seam_camera
from cpu_builds import cpu_buoyancy, cpu_buoyancy_moving, cpu_query, cpu_query_velocity, cpu_raycast, cpu_render, CpuSet
from cpu_builds import bodies_harness, buoyancy_harness, query_harness, raycast_harness, render_harness, velocity_harness  # noqa: F401 (fixtures)
from scenes import demo_bodies, gpu_arrays, gpu_maps, mixed_rays, query_points, SUN_BEHIND, velocity_layers as _vel_layers

REC = W.SURFACE_QUERY
SLAB_FLOOR = np.float32(1e-2)   # csrc/ow_raycast.h kSlabFloor


def edge_context(n, count, ticks=3, bodies_kernels=None):
    gen = W()
    gen.map_size = n
    gen.bodies_kernels = bodies_kernels
    gen.init_gpu(max(2, count))
    gen.run(UPDATE_DELTA, [WaveCascadeParameters(**r) for r in E.edge_records()[:count]], ticks)
    sc = E.EDGE_SCALES[:count]
    d, m = gpu_maps(gen, count)
    return gen, sc, d, m


def edge_points(sc, n, count):
    far, bad = E.far_points()
    xz = np.concatenate([E.seam_points(sc, n), far, bad, query_points(count, seed=n)])
    c0, r0 = E.tap_integers(sc, n, E.seam_points(sc, n))
    assert ((c0 == n - 1).any(axis=1) & (r0 == n - 1).any(axis=1)).all()   # every cascade has taps on its last column and its last row
    return xz, len(far), len(bad)


def seam_rays(sc, n):
    """rays that start above a seam point and look down, and rays that run along the seam x = -0.25 texels of each cascade at a grazing
    angle (every sample's tap has c0 = n - 1 in that cascade)"""
    pts = E.seam_points(sc, n)[::3]
    o = np.stack([pts[:, 0], np.full(len(pts), 12.0, np.float32), pts[:, 1]], axis=1)
    down = W.rays(o, np.tile([(0.05, -1.0, -0.03)], (len(o), 1)), 200.0)
    along_o = np.array([(-0.25 / (sx * n), 6.0, -40.0) for sx, _, _, _ in sc], np.float32)
    along = W.rays(along_o, np.tile([(0.0, -0.08, 1.0)], (len(along_o), 1)), 400.0)
    return np.concatenate([down, along])


def edge_hulls(sc, n, seed=0):
    """24 bodies with hulls of 1, 63, 64, 65 and 200 points in turn; bodies 3 and 4 on seam points, body 5 at 1e7 m"""
    rng = np.random.default_rng(seed)
    counts = [(1, 63, 64, 65, 200)[i % 5] for i in range(24)]
    bodies = np.zeros(24, W.BUOYANCY_BODY)
    hull = np.zeros(sum(counts), W.HULL_POINT)
    seams = E.seam_points(sc, n)
    off = 0
    for i, c in enumerate(counts):
        bodies[i]["transform"][:9] = np.eye(3, dtype=np.float32).ravel()
        bodies[i]["transform"][9:] = (rng.uniform(-200, 200), rng.uniform(-1.0, 0.5), rng.uniform(-200, 200))
        bodies[i]["linear_velocity"] = rng.normal(0, 1, 3)
        bodies[i]["angular_velocity"] = rng.normal(0, 0.2, 3)
        bodies[i]["linear_drag"], bodies[i]["quadratic_drag"] = 0.3, 0.1
        bodies[i]["point_offset"], bodies[i]["point_count"] = off, c
        hull["local"][off:off + c] = rng.uniform(-1, 1, (c, 3)) * (3.0, 0.6, 3.0)
        hull["volume"][off:off + c], hull["half_height"][off:off + c], hull["body"][off:off + c] = 0.4, 0.25, i
        off += c
    bodies[3]["transform"][[9, 11]] = seams[2]
    bodies[4]["transform"][[9, 11]] = seams[len(seams) // 2 + 2]
    hull["local"][bodies[3]["point_offset"]] = 0.0      # a hull point exactly on the seam point
    bodies[5]["transform"][[9, 11]] = (1e7, -1e7)
    return bodies, hull


@pytest.fixture(scope="module")
def context256():
    return edge_context(256, 5)


@pytest.mark.gpu
def test_sampling_on_edge_scales_is_the_oracles_bit_for_bit(context256):
    gen, sc, d, m = context256
    xz, _, _ = edge_points(sc, 256, 4000)
    got = gen.sample_surface(xz, sc)
    want = O.sample_surface(d, m, sc, xz)
    for f in O.SURFACE_SAMPLE.names:
        assert got[f].tobytes() == want[f].tobytes(), f
    float_fields_finite(got)
    assert np.abs(got["displacement"]).max() > 0.1


@pytest.mark.gpu
def test_query_and_velocity_on_edge_scales_are_the_cpu_builds_bit_for_bit(context256, query_harness, velocity_harness):
    gen, sc, d, m = context256
    xz, nfar, nbad = edge_points(sc, 256, 4000)
    first_far = len(xz) - 4000 - nbad - nfar
    for kw in OPTION_SETS:
        got = gen.query_surface(xz, sc, kw or None)
        want = cpu_query(query_harness, d, m, sc, xz, **kw)
        for f in REC.names:
            if f != "world_xz":   # the echo of a NaN q compares as bytes too, but say which field
                assert got[f].tobytes() == want[f].tobytes(), (kw, f)
        assert got["world_xz"].tobytes() == xz.tobytes()
        finite_q = np.isfinite(xz).all(axis=1)
        float_fields_finite(got[finite_q])
        assert np.isfinite(got["height"]).all() and np.isfinite(got["sample"]["displacement"]).all()
        far = got[first_far:first_far + nfar]
        assert set(np.unique(far["converged"])) <= {0, 1} and (far["iterations"] <= (kw.get("max_iterations") or 16)).all()
        bad = got[first_far + nfar:first_far + nfar + nbad]
        assert (bad["p"] == 0).all() and (bad["converged"] == 0).all()
    v = _vel_layers(gen, len(sc))
    for opts, center in ((None, None), ({"falloff_center": (12.5, -40.0)}, (12.5, -40.0))):
        got = gen.query_velocity(xz, sc, opts)
        want = cpu_query_velocity(velocity_harness, d, v, sc, xz, center)
        assert got.tobytes() == want.tobytes()
        float_fields_finite(got)
        assert np.abs(got["velocity"]).max() > 1e-2


@pytest.mark.gpu
def test_buoyancy_on_edge_scales_is_the_cpu_builds_bit_for_bit(context256, buoyancy_harness, velocity_harness):
    gen, sc, d, m = context256
    bodies, hull = edge_hulls(sc, 256)
    got_pts = np.zeros(len(hull), W.BUOYANCY_POINT)
    got = gen.buoyancy(bodies, hull, sc, None, points=got_pts)
    want, want_pts = cpu_buoyancy(buoyancy_harness, d, sc, bodies, hull, {})
    assert got_pts.tobytes() == want_pts.tobytes() and got.tobytes() == want.tobytes()
    float_fields_finite(got)
    float_fields_finite(got_pts)
    moved = bodies.copy()
    moved["transform"][:, 9:] += np.random.default_rng(1).normal(0, 0.4, (len(bodies), 3)).astype(np.float32)
    got_w = gen.buoyancy(moved, hull, sc, {"warm_start": True}, points=got_pts)
    want_w, want_pts = cpu_buoyancy(buoyancy_harness, d, sc, moved, hull, {"warm_start": True}, points=want_pts)
    assert got_pts.tobytes() == want_pts.tobytes() and got_w.tobytes() == want_w.tobytes()
    pts2 = np.zeros(len(hull), W.BUOYANCY_POINT)
    got2 = gen.buoyancy(bodies, hull, sc, {"water_velocity": True}, pts2)
    want2, wpts2 = cpu_buoyancy_moving(velocity_harness, d, _vel_layers(gen, len(sc)), sc, bodies, hull)
    assert got2.tobytes() == want2.tobytes() and pts2.tobytes() == wpts2.tobytes()
    assert got2.tobytes() != got.tobytes() and (got["wetted_points"] > 0).sum() > 5


@pytest.mark.gpu
def test_ray_casts_on_edge_scales_are_the_cpu_builds_bit_for_bit(context256, raycast_harness):
    gen, sc, d, m = context256
    rays = np.concatenate([mixed_rays(256)[::4], seam_rays(sc, 256)])
    for opts in (None, {"falloff_center": (12.5, -40.0)}):
        got = gen.raycast_surface(rays, sc, opts)
        want = cpu_raycast(raycast_harness, d, m, sc, rays, opts)
        for f in W.RAYCAST_HIT.names:
            assert got[f].tobytes() == want[f].tobytes(), (opts, f)
    assert ((got["status"] & 1) != 0).mean() > 0.3


@pytest.mark.gpu
def test_render_view_above_a_seam_is_the_cpu_builds_bit_for_bit(context256, render_harness):
    """48 x 32 (six by four tiles of 8 x 8 pixels) from a camera above a point on the last column and row of cascade 0's tile"""
    gen, sc, d, m = context256
    cam = seam_camera(sc, 256, width=48, height=32)
    for what, opts in (("defaults", None), ("falloff", {"falloff": True, "roughness": 0.4, "light_direction": SUN_BEHIND})):
        got = gen.render_view(cam, sc, opts)
        want = cpu_render(render_harness, d, m, sc, cam, opts)
        assert_same_image(got, want, what)
        assert ((got[1]["status"] & 1) != 0).mean() > 0.3, what
        only_rgba, none = gen.render_view(cam, sc, opts, pixels=False)
        assert none is None and only_rgba.tobytes() == want[0].tobytes(), what


def edge_rigid_bodies(sc, n):
    """free bodies of 1, 63, 64, 65 and 200 hull points; body 1 starts on a seam point, body 3 at 1e7 m"""
    st, hull = demo_bodies(counts=(1, 63, 64, 65, 200), seed=7, spread=120.0)
    x, z = E.seam_points(sc, n)[2]
    st["position"][1, 0], st["position"][1, 2] = float(x), float(z)
    st["position"][3, 0], st["position"][3, 2] = 1e7, -1e7
    return st, hull


@pytest.mark.gpu
@pytest.mark.parametrize("kernels", ["fused", "split"])
def test_bodies_step_on_edge_scales_is_the_cpu_builds_bit_for_bit(bodies_harness, kernels):
    """k_bodies_step (fused) and k_buoyancy_points + k_bodies_integrate (split), 4 substeps and 4 more, on EDGE_SCALES at 256^2"""
    gen, sc, d, m = edge_context(256, 5, bodies_kernels=kernels)
    gen.update_velocity()
    vel = _vel_layers(gen, len(sc))
    st, hull = edge_rigid_bodies(sc, 256)
    for opts in ({}, {"warm_start": True, "water_velocity": True}):
        v = vel if opts.get("water_velocity") else None
        s = gen.bodies_create(st, hull)
        cs = CpuSet(bodies_harness, st, hull)
        for call in range(2):
            gen.bodies_step(s, sc, 4, 1.0 / 120.0, opts)
            cs.step(d, sc, 4, 1.0 / 120.0, opts, vel=v)
            got, want = gpu_arrays(gen, s), cs.arrays()
            for name in want:
                assert got[name] == want[name], (opts, call, name)
        stats = gen.bodies_stats(s)
        assert stats["faulted_bodies"] == 0 and (stats["fused_launches"], stats["split_calls"]) == ((2, 0) if kernels == "fused" else (0, 2))
        gen.bodies_destroy(s)
    moved = np.frombuffer(want["state"], W.RIGID_BODY)
    assert np.isfinite(moved["position"]).all() and np.abs(moved["position"] - st["position"]).max() > 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("n,count", [(1024, 2), (2048, 1)])
def test_large_maps_on_non_square_tiles(query_harness, raycast_harness, n, count):
    """the sample / query / cast subset at the sizes whose rows are wide: a seam tap's two rows lie 16 KiB apart at 2048^2"""
    gen, sc, d, m = edge_context(n, count)
    xz, _, _ = edge_points(sc, n, 2000)
    assert len(xz) <= 3000
    got = gen.sample_surface(xz, sc)
    want = O.sample_surface(d, m, sc, xz)
    for f in O.SURFACE_SAMPLE.names:
        assert got[f].tobytes() == want[f].tobytes(), f
    for kw in OPTION_SETS[:2]:
        got = gen.query_surface(xz, sc, kw or None)
        want = cpu_query(query_harness, d, m, sc, xz, **kw)
        assert got.tobytes() == want.tobytes(), kw
    rays = np.concatenate([mixed_rays(n)[::10], seam_rays(sc, n)])[:256]
    got = gen.raycast_surface(rays, sc, None)
    want = cpu_raycast(raycast_harness, d, m, sc, rays, None)
    assert got.tobytes() == want.tobytes()


def slab_from_maps(d, sc):
    """csrc/ow_raycast.h step 1 from the maps read back: per layer the largest FP16 magnitude of D_y (the maximum over the bits with the
    sign cleared), times |scales.z|, summed in cascade order in FP32, widened by 2^-10 and the floor"""
    H = np.float32(0)
    for i in range(len(sc)):
        bits = (np.asarray(d[i]).view(np.uint16)[..., 1] & 0x7FFF).max()
        H = np.float32(H + np.array([bits], np.uint16).view(np.float16).astype(np.float32)[0] * np.abs(np.float32(sc[i, 2])))
    return np.float32(H * np.float32(1.0 + 0.0009765625) + SLAB_FLOOR)


def write_displacement_layers(gen, layers):
    """crafted displacement layers [count][n][n][4] FP16 copied over the context's own (ow_get_device_ptrs: layer i at rid + i * stride)"""
    gen.sync()
    desc = gen.descriptors["displacement_map"]
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    n = gen.map_size
    for i, layer in enumerate(layers):
        bits = np.ascontiguousarray(layer, np.float16)
        assert bits.shape == (n, n, 4) and bits.nbytes == n * n * 8 <= desc.layer_stride and i < gen.num_cascades
        assert hip.hipMemcpy(desc.rid + i * desc.layer_stride, bits.ctypes.data, bits.nbytes, 1) == 0   # host to device


@pytest.mark.gpu
def test_height_bound_through_the_cast():
    """k_height_bound's words are not exported: a vertical ray from above reports the slab it was given (slab_half_height) and enters it
    at the analytic t.  On the pipeline's maps, with the scale's sign flipped (the same slab), and after more ticks (the words are
    cleared and rebuilt in stream order); then on crafted layers whose largest |D_y| sits in texel 0 -- the first element of the
    reduction -- and in texel N^2 - 1, the last, with either sign, every other texel far smaller."""
    gen, sc, d, m = edge_context(256, 5)
    ray = W.rays([(3.0, 500.0, -4.0)], [(0.0, -1.0, 0.0)], 2000.0)

    def check(scales, hw):
        out = gen.raycast_surface(ray, scales, None)
        assert out["slab_half_height"][0] == hw
        assert out["t_enter"][0] == np.float32(np.float32(np.float32(0.0) + hw) - np.float32(500.0)) / np.float32(-1.0)

    flipped = sc.copy()
    flipped[:, 2] = -flipped[:, 2]
    hw = slab_from_maps(d, sc)
    assert hw > 0.5
    check(sc, hw)
    check(flipped, hw)
    gen.run(UPDATE_DELTA, [WaveCascadeParameters(**r) for r in E.edge_records()], 7)
    d2, _ = gpu_maps(gen, len(sc))
    hw2 = slab_from_maps(d2, sc)
    assert hw2 != hw
    check(sc, hw2)
    rng = np.random.default_rng(3)
    two = sc[:2].copy()
    two[:, 2] = (1.0, -0.5)
    for index in (0, 256 * 256 - 1):
        layers = rng.uniform(-0.25, 0.25, (2, 256, 256, 4)).astype(np.float16)
        layers[..., 0] = 9.0          # D_x and D_z larger than any D_y: the bound reads the y channel alone
        layers[..., 2] = -9.0
        layers.reshape(2, -1, 4)[0, index, 1] = 3.0
        layers.reshape(2, -1, 4)[1, index, 1] = -2.5
        write_displacement_layers(gen, layers)
        back, _ = gpu_maps(gen, 2)
        assert np.asarray(back).view(np.uint16).tobytes() == layers.view(np.uint16).tobytes()
        want = np.float32(np.float32(np.float32(3.0) + np.float32(2.5) * np.float32(0.5)) * np.float32(1.0 + 0.0009765625) + SLAB_FLOOR)
        assert slab_from_maps(layers, two) == want
        check(two, want)
        other = two.copy()
        other[:, 2] = (-1.0, 0.5)
        check(other, want)

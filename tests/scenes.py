"""Scenes and inputs of the suite, and of the programs under scripts/ that time the same scenes: contexts and maps, cameras, meshes and
shapes, bodies, textures and panoramas, the whole-frame scene, and the constants several modules share.  Nothing here asserts and nothing
here builds: the CPU builds are in tests/cpu_builds.py, the comparisons in tests/checks.py."""
import ctypes as C
import math

import numpy as np

import helpers as H
from godotoceanwaves_amd import _lib
from godotoceanwaves_amd.presets import cascade_preset, UPDATE_DELTA
from godotoceanwaves_amd.wave_generator import WaveGenerator, WaveGenerator as W

SOLID, ENV = _lib.OW_RAY_SOLID, _lib.OW_RAY_ENVIRONMENT


SCALES3 = np.array([[1 / 88, 1 / 88, 1.0, 1.0], [1 / 57, 1 / 57, 0.75, 0.5], [1 / 16, 1 / 16, 0.5, 0.25]], np.float32)


def random_maps(C, N, seed=0, foam_hi=0.6):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((C, N, N, 4)).astype(np.float16)
    m = (rng.standard_normal((C, N, N, 4)) * 0.3).astype(np.float16)
    m[..., 3] = rng.uniform(0, foam_hi, (C, N, N)).astype(np.float16)
    return d, m


def query_points(count, seed=1, span=700.0):
    """random points plus the awkward ones: origin, texel centres and edges, negative coordinates, far away"""
    rng = np.random.default_rng(seed)
    xz = rng.uniform(-span, span, (count, 2)).astype(np.float32)
    xz[:8] = [[0, 0], [88 / 256 * 0.5, 88 / 256 * 0.5], [88.0, 88.0], [-88.0, 57.0], [-0.001, -0.001], [1e4, -1e4], [16.0, -16.0], [44.0, 28.5]]
    return xz


FIELDS_PINNED = ["displacement", "gradient", "foam", "normal_factor", "foam_factor", "scale_factor", "spray_active",
                 "gradient_fragment", "foam_fragment"]


def sampling_case(case):
    """maps, scales and query points of one case of the test below (tests/golden/make_ref_digests.py samples the same)"""
    sc = SCALES3
    if case == "random_maps":
        d, m = random_maps(3, 64)
    elif case == "spray_active":  # foam near 1 and flat normals: ACTIVE both ways, both factor branches
        d, m = random_maps(3, 32, seed=5, foam_hi=0.7)
        m[..., :2] *= np.float16(0.1)
    elif case == "fine_cascades":  # ppm * 0.1 >= 1 on every cascade: the mix takes the bilinear lookup alone
        d, m = random_maps(3, 64, seed=7)
        sc = np.array([[1 / 5, 1 / 4, 1.0, 1.3], [1 / 3, 1 / 6, 0.75, 0.5], [1 / 2, 1 / 2, 0.5, 0.25]], np.float32)
    else:  # maps the pipeline itself produced (oracle generator), three cascades
        g = H.oracle_generator(128, [0, 1, 2])
        for _ in range(2):
            g.update_all(UPDATE_DELTA)
        d = np.stack([g.displacement(i) for i in range(3)])
        m = np.stack([g.normal(i) for i in range(3)])
    return d, m, sc, query_points(3000, seed=11)


def ref_sampling_digests(r, dp):
    """what the reference's shader text computed for one case: FIELDS_PINNED and the particle shader's displacement sum"""
    return {**{f: H.digest(r[f]) for f in FIELDS_PINNED}, "particle_displacement": H.digest(dp)}


def maps_u16(maps):
    m = np.ascontiguousarray(np.asarray(maps))
    return m.view(np.uint16) if m.dtype != np.uint16 else m


def generated_maps(n, ids, ticks=2):
    g = H.oracle_generator(n, ids, native=True)
    for _ in range(ticks):
        g.update_all(UPDATE_DELTA)
    d = np.stack([np.asarray(g.displacement(i)) for i in range(len(ids))])
    m = np.stack([np.asarray(g.normal(i)) for i in range(len(ids))])
    sc = np.array([(1 / cascade_preset(ci)["tile_length"][0], 1 / cascade_preset(ci)["tile_length"][1], 1.0, 1.0) for ci in ids], np.float32)
    return maps_u16(d), maps_u16(m), sc


def make_gen(n, ids, stream=None):
    from godotoceanwaves_amd import WaveCascadeParameters
    gen = WaveGenerator()
    gen.map_size = n
    if stream is not None:
        gen.stream = stream
    gen.init_gpu(max(2, len(ids)))
    return gen, [WaveCascadeParameters(**cascade_preset(ci)) for ci in ids]


def scales_of(params):
    return np.array([(1 / p.tile_length[0], 1 / p.tile_length[1], p.displacement_scale, p.normal_scale) for p in params], np.float32)


def gpu_maps(gen, count):
    maps = [gen.get_maps(i) for i in range(count)]
    return np.stack([mp[0] for mp in maps]), np.stack([mp[1] for mp in maps])


GROW_POINTS = (16, 4097, 16)   # under the scratch's floor of 4 096 points, one past it (the block is replaced), under it again (the larger block stays)


def smallest_context():
    """128^2 x 2, three ticks in: (generator, map scales, displacement, normal maps)"""
    gen, params = make_gen(128, [0, 1])
    gen.run(UPDATE_DELTA, params, 3)
    return (gen, scales_of(params)) + gpu_maps(gen, 2)


HIT, BELOW, TRUNC, INVALID = _lib.OW_RAY_HIT, _lib.OW_RAY_FROM_BELOW, _lib.OW_RAY_TRUNCATED, _lib.OW_RAY_INVALID


SPACING, RAY_TOL = 0.25, 1e-3


def unit(d):
    d = np.asarray(d, np.float32)
    return d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]


def camera_rays(count, heights, angles, seed, span=200.0, max_distance=2000.0):
    """rays from (x, y, z), y in heights, x and z in [-span, span], pointing down by a depression angle in `angles` (degrees) at a random
    azimuth"""
    rng = np.random.default_rng(seed)
    h = rng.uniform(*heights, count)
    a = np.radians(rng.uniform(*angles, count))
    az = rng.uniform(0, 2 * np.pi, count)
    o = np.stack([rng.uniform(-span, span, count), h, rng.uniform(-span, span, count)], axis=1)
    return W.rays(o, np.stack([np.cos(a) * np.cos(az), -np.sin(a), np.cos(a) * np.sin(az)], axis=1), max_distance)


def calm_maps(n=64, cascades=2):
    return np.zeros((cascades, n, n, 4), np.uint16), np.zeros((cascades, n, n, 4), np.uint16), np.array([(1 / 50.0, 1 / 50.0, 1.0, 1.0)] * cascades,
                                                                                                            np.float32)


def calm_hit_rays(wl):
    """400 rays onto a calm sea at water level wl, half of them at 45 degrees and half steeper, from 0.5 m to 200 m above it, their
    directions of any length: (rays, heights above the water)"""
    rng = np.random.default_rng(1)
    R = 400
    ang = np.radians(np.concatenate([np.full(R // 2, 45.0), rng.uniform(60.0, 90.0, R // 2)]))
    az = rng.uniform(0, 2 * np.pi, R)
    h = rng.uniform(0.5, 200.0, R)
    o = np.stack([rng.uniform(-300, 300, R), wl + h, rng.uniform(-300, 300, R)], axis=1)
    return W.rays(o, np.stack([np.cos(ang) * np.cos(az), -np.sin(ang), np.cos(ang) * np.sin(az)], axis=1) * rng.uniform(0.1, 30.0, (R, 1)), 1000.0), h


def calm_miss_rays(wl):
    """nine rays round a calm sea at water level wl: misses above and below the slab, hits from above and below, truncation inside it"""
    return W.rays([(0, 5, 0), (3, 50, 3), (0, 5, 0), (10, 0.02 + wl, 0), (0, -3, 0), (0, -3, 0), (0, -0.005 + wl, 0), (0, 20, 0), (0, wl, 0)],
                  [(0, 1, 0), (1, 0, 0), (1, -1, 0), (1, 0, 0), (0, 1, 1), (0, -1, 0), (1, 0, 0), (0, -1, 0), (1, 0, 0)],
                  [100, 100, 100, 100, 100, 100, 5000, 10, 100])


def swell_rays():
    return camera_rays(300, (2.0, 60.0), (3.0, 80.0), seed=11, max_distance=3000.0)


def swell_maps(n=256, tile=100.0, amplitude=1.5, wavelength=20.0):
    """D_xz = 0, D_y = A cos(k x) at the texel centres, in FP16: a height-only swell (the query's p is q)"""
    x = (np.arange(n) + 0.5) * tile / n
    d = np.zeros((1, n, n, 4), np.float16)
    d[0, :, :, 1] = (amplitude * np.cos(2 * np.pi * x / wavelength))[None, :]
    return maps_u16(d), np.zeros((1, n, n, 4), np.uint16), np.array([(1 / tile, 1 / tile, 1.0, 1.0)], np.float32)


def slope_factor(d, max_slope):
    """|dg/dt| <= |d.y| + max_slope |d.xz| along a unit direction: how far g can move per metre of ray"""
    d = np.asarray(d, np.float64)
    return np.abs(d[:, 1]) + max_slope * np.hypot(d[:, 0], d[:, 2])


def mixed_rays(seed):
    a = camera_rays(1500, (2, 300), (2, 80), seed=seed)
    b = camera_rays(500, (2, 20), (2, 10), seed=seed + 1)
    c = W.rays([(0, 10, 0), (0, -3, 0), (0, 0.3, 0), (np.nan, 0, 0), (4, 50, 4)], [(1, -1, 0), (0, 1, 0), (1, 0, 0), (0, -1, 0), (0, 0, 0)],
               [100, 100, 5000, 10, 10])
    return np.concatenate([a, b, c])


RHO, G = 1025.0, 9.81


RHO_G = float(np.float32(RHO) * np.float32(G))


def rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


def make_scene(boxes):
    """boxes: dicts of origin, basis (3x3), size, divisions and optional v / w / kl / kq -> (bodies, hull)"""
    bodies = np.zeros(len(boxes), W.BUOYANCY_BODY)
    hulls, off = [], 0
    for i, bx in enumerate(boxes):
        h = W.box_hull(bx["size"], bx["divisions"], body=i)
        bodies[i]["transform"][:9] = np.asarray(bx.get("basis", np.eye(3)), np.float32).ravel()
        bodies[i]["transform"][9:] = bx["origin"]
        bodies[i]["linear_velocity"] = bx.get("v", (0, 0, 0))
        bodies[i]["angular_velocity"] = bx.get("w", (0, 0, 0))
        bodies[i]["linear_drag"] = bx.get("kl", 0.0)
        bodies[i]["quadratic_drag"] = bx.get("kq", 0.0)
        bodies[i]["point_offset"], bodies[i]["point_count"] = off, len(h)
        hulls.append(h)
        off += len(h)
    return bodies, np.concatenate(hulls) if hulls else np.zeros(0, W.HULL_POINT)


def calm(n=64, cascades=1):
    """maps of any content with map_scales.z = 0: no displacement, the surface is the plane y = water_level"""
    rng = np.random.default_rng(0)
    d = rng.normal(0, 1, (cascades, n, n, 4)).astype(np.float16)
    sc = np.array([(1 / 50.0, 1 / 50.0, 0.0, 1.0)] * cascades, np.float32)
    return maps_u16(d), sc


def demo_scene(count=12, seed=0, spread=300.0, divisions=(4, 3, 6)):
    rng = np.random.default_rng(seed)
    boxes = []
    for i in range(count):
        R = rotation(rng.normal(size=3), rng.uniform(-0.6, 0.6))
        boxes.append(dict(origin=(rng.uniform(-spread, spread), rng.uniform(-1.5, 1.0), rng.uniform(-spread, spread)), basis=R,
                          size=(rng.uniform(2, 8), rng.uniform(1, 3), rng.uniform(4, 15)), divisions=divisions,
                          v=rng.normal(0, 1, 3), w=rng.normal(0, 0.2, 3), kl=0.3, kq=0.1))
    return make_scene(boxes)


def bilinear64(layer, u, v):
    n = layer.shape[0]
    fx, fy = u * n - 0.5, v * n - 0.5
    x0, y0 = np.floor(fx), np.floor(fy)
    wx, wy = (fx - x0)[:, None], (fy - y0)[:, None]
    c0, r0 = x0.astype(np.int64) % n, y0.astype(np.int64) % n
    c1, r1 = (c0 + 1) % n, (r0 + 1) % n
    L = layer.astype(np.float64)
    return (L[r0, c0] * (1 - wx) + L[r0, c1] * wx) * (1 - wy) + (L[r1, c0] * (1 - wx) + L[r1, c1] * wx) * wy


def velocity_layers(gen, count):
    return np.stack([gen.velocity_map(i) for i in range(count)])


def quaternion(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    q = np.concatenate([a * np.sin(angle / 2), [np.cos(angle / 2)]])
    return q / np.sqrt((q * q).sum())


def blob_hull(count, size, body, seed):
    """`count` hull points scattered in a box of `size`: the volume shared evenly, half heights of a cell of that volume"""
    rng = np.random.default_rng(seed)
    h = np.zeros(count, W.HULL_POINT)
    h["local"] = rng.uniform(-0.5, 0.5, (count, 3)) * np.asarray(size)
    h["volume"] = np.prod(size) / max(count, 1)
    h["half_height"] = 0.5 * (np.prod(size) / max(count, 1)) ** (1 / 3)
    h["body"] = body
    return h


def make_bodies(items):
    """items: dicts of hull (HULL_POINT records of this body), size, and optional origin, q, v, w, density (of the body; 0: kinematic), kl, kq,
    force, torque -> (RIGID_BODY records, hull)"""
    st = np.zeros(len(items), W.RIGID_BODY)
    hulls, off = [], 0
    for i, it in enumerate(items):
        h = it["hull"].copy()
        h["body"] = i
        st[i]["position"] = it.get("origin", (0, 0, 0))
        st[i]["orientation"] = it.get("q", (0, 0, 0, 1))
        st[i]["linear_velocity"] = it.get("v", (0, 0, 0))
        st[i]["angular_velocity"] = it.get("w", (0, 0, 0))
        dens = it.get("density", 0.5 * RHO)
        if dens > 0:
            m, iinv = W.box_mass_properties(it["size"], dens)
            st[i]["mass"], st[i]["inverse_inertia"] = m, iinv
        st[i]["applied_force"] = it.get("force", (0, 0, 0))
        st[i]["applied_torque"] = it.get("torque", (0, 0, 0))
        st[i]["linear_drag"], st[i]["quadratic_drag"] = it.get("kl", 0.0), it.get("kq", 0.0)
        st[i]["point_offset"], st[i]["point_count"] = off, len(h)
        hulls.append(h)
        off += len(h)
    return st, (np.concatenate(hulls) if hulls else np.zeros(0, W.HULL_POINT))


def crate(size=(2, 1, 2), divisions=(4, 4, 4), **kw):
    return dict(hull=W.box_hull(size, divisions), size=size, **kw)


def demo_bodies(counts=(64, 36, 72, 48), seed=0, spread=200.0):
    rng = np.random.default_rng(seed)
    items = []
    for i, c in enumerate(counts):
        size = (rng.uniform(2, 6), rng.uniform(1, 2), rng.uniform(3, 8))
        items.append(dict(hull=blob_hull(c, size, i, seed * 100 + i), size=size, origin=(rng.uniform(-spread, spread), rng.uniform(-0.5, 0.8), rng.uniform(-spread, spread)),
                          q=quaternion(rng.normal(size=3), rng.uniform(-0.6, 0.6)), v=rng.normal(0, 1, 3), w=rng.normal(0, 0.3, 3), kl=0.6, kq=0.2,
                          density=rng.uniform(300, 700), force=(rng.normal(0, 200), 0, rng.normal(0, 200)), torque=rng.normal(0, 50, 3)))
    return make_bodies(items)


PARITY_COUNTS = (1, 63, 64, 65, 200, 1000, 30)   # hull points per body: one, around a wave of 64, many; seven bodies span two blocks of four


HALF_Q = (0.5, 0.5, 0.5, 0.5)   # R = [0 0 1; 1 0 0; 0 1 0] exactly: body x -> world y, y -> z, z -> x


def random_rigid_states(count, seed):
    """(RIGID_BODY records, BUOYANCY_RESULT records, dt per case) for single substeps: random unit q (every sixteenth of length 0.5, every
    sixteenth of length 2), v, w, Fa, Ta, FP32 force and torque records of both signs from 1 to 1e4, masses from 10 to 5000, distinct Iinv,
    every fifth case with one axis locked, dt cycling through 1/240, 1/60 and 0.1.  No hull: the records stand for it"""
    rng = np.random.default_rng(seed)
    st, res = np.zeros(count, W.RIGID_BODY), np.zeros(count, W.BUOYANCY_RESULT)
    q = rng.normal(size=(count, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    q[3::16] *= 0.5
    q[11::16] *= 2.0
    st["orientation"] = q
    st["position"] = rng.uniform(-500, 500, (count, 3))
    st["linear_velocity"], st["angular_velocity"] = rng.normal(0, 5, (count, 3)), rng.normal(0, 2, (count, 3))
    st["mass"] = rng.uniform(10, 5000, count)
    st["inverse_inertia"] = 10.0 ** rng.uniform(-4, -1, (count, 3))
    for i in range(0, count, 5):
        st["inverse_inertia"][i, (i // 5) % 3] = 0.0
    st["applied_force"], st["applied_torque"] = rng.normal(0, 1e3, (count, 3)), rng.normal(0, 300, (count, 3))
    st["linear_drag"], st["quadratic_drag"] = 0.6, 0.2
    sign = lambda: rng.choice([-1.0, 1.0], (count, 3))   # noqa: E731
    res["force"] = (sign() * 10.0 ** rng.uniform(0, 4, (count, 3))).astype(np.float32)
    res["torque"] = (sign() * 10.0 ** rng.uniform(0, 4, (count, 3))).astype(np.float32)
    dts = np.array([1.0 / 240.0, 1.0 / 60.0, 0.1])[np.arange(count) % 3]
    return st, res, dts


def seven_bodies(seed, height=None, spread=120.0):
    """demo_bodies with PARITY_COUNTS hull points, body 6 kinematic and body 2 with its y axis locked; height: all of them that far up"""
    st, hull = demo_bodies(counts=PARITY_COUNTS, seed=seed, spread=spread)
    st["mass"][6] = 0.0
    st["inverse_inertia"][2, 1] = 0.0
    if height is not None:
        st["position"][:, 1] = height
    return st, hull


def airborne_bodies(seed=21):
    """seven_bodies 1000 m up with any unit orientation, spinning, pushed and twisted by applied loads"""
    st, hull = seven_bodies(seed, height=1000.0)
    rng = np.random.default_rng(seed + 1)
    q = rng.normal(size=(len(st), 4))
    st["orientation"] = q / np.linalg.norm(q, axis=1)[:, None]
    st["angular_velocity"] = rng.normal(0, 2, (len(st), 3))
    st["applied_force"], st["applied_torque"] = rng.normal(0, 1e3, (len(st), 3)), rng.normal(0, 300, (len(st), 3))
    return st, hull


BASIS_IINV = (0.375, 0.0625, 1.75)      # a, b, c: distinct, and exact in binary


BASIS_TORQUE = 123.456


def basis_bodies():
    """seven bodies at rest at HALF_Q, 1000 m up, one applied torque each: (states, hull, per body the world axis of the torque, the body axis
    whose Iinv it must meet, and whether that axis is locked).  Body 6 is kinematic"""
    st, hull = seven_bodies(5, height=1000.0)
    cases = [(1, 0, False), (2, 1, False), (0, 2, False), (1, 0, True), (2, 1, True), (1, 0, False), (1, 0, False)]
    for b, (world, body, locked) in enumerate(cases):
        st["orientation"][b] = HALF_Q
        st["linear_velocity"][b] = st["angular_velocity"][b] = st["applied_force"][b] = st["applied_torque"][b] = 0.0
        st["inverse_inertia"][b] = BASIS_IINV
        if locked:
            st["inverse_inertia"][b, body] = 0.0
        st["applied_torque"][b, world] = BASIS_TORQUE if b != 5 else -BASIS_TORQUE
    return st, hull, cases


SPIN_Q0, SPIN_W = ((1, 2, 3), 0.7), (1.1, -2.3, 0.7)


def spin_bodies():
    """seven bodies spinning freely 10^6 m up (no applied load, no contact): body 0 is SPIN_Q0 / SPIN_W, the others other axes and rates; body 2
    has an axis locked (no torque ever meets it) and body 6 is kinematic"""
    st, hull = seven_bodies(9, height=1e6)
    rng = np.random.default_rng(10)
    for b in range(len(st)):
        st["orientation"][b] = quaternion(*SPIN_Q0) if b == 0 else quaternion(rng.normal(size=3), rng.uniform(-3, 3))
        st["angular_velocity"][b] = SPIN_W if b == 0 else rng.normal(0, 2, 3)
        st["linear_velocity"][b] = st["applied_force"][b] = st["applied_torque"][b] = 0.0
    return st, hull


def saturated_bodies():
    """three crates whose FP64 state is finite and beyond FP32: far out, one moving and one spinning faster than FP32 holds"""
    st, hull = make_bodies([crate(origin=(1e39, 0.0, -1e39), divisions=(2, 2, 2), kl=3.0, kq=0.5),
                            crate(origin=(3.5e38, 0.0, 0.0), divisions=(2, 2, 2), v=(1e39, 0, 0), kl=3.0, kq=0.5),
                            crate(origin=(0.0, -1e39, 0.0), divisions=(2, 2, 2), w=(0, -1e39, 0), kl=3.0, kq=0.5)])
    return st, hull


TILT_SIZE = (2.0, 0.5, 2.0)


def tilted_box(axis, angle):
    """a wide, flat box of half the water's density at its Archimedes draft (its centre on the calm surface), at rest, tilted about `axis`"""
    return make_bodies([crate(size=TILT_SIZE, divisions=(6, 4, 6), origin=(0.0, 0.0, 0.0), q=quaternion(axis, angle), kl=3.0, kq=0.5)])


def hip():
    h = C.CDLL("libamdhip64.so")
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    h.hipStreamSynchronize.argtypes = [C.c_void_p]
    return h


def device_read(ptr, count, dtype, stream=None):
    out = np.zeros(count, dtype)
    if count == 0:
        return out
    if stream is None:
        assert hip().hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
    else:   # through the caller's stream only
        assert hip().hipMemcpyAsync(out.ctypes.data, ptr, out.nbytes, 2, stream) == 0
        assert hip().hipStreamSynchronize(stream) == 0
    return out


def device_array(ptr, shape, dtype):
    return device_read(ptr, int(np.prod(shape)), dtype).reshape(shape)


def gpu_mesh_draw(gen, mesh_handle, cam, origin, sc, options=None):
    """ow_mesh_draw and what it left resident, in cpu_mesh_draw's form: rgba, rec, vertices, vis and the four counters"""
    rgba, rec = gen.mesh_draw(mesh_handle, cam, origin, sc, options)
    vptr, wptr = gen.mesh_device_ptrs(mesh_handle)
    stats = gen.mesh_stats(mesh_handle)
    return dict(rgba=rgba, rec=rec, vertices=device_array(vptr, mesh_handle.num_vertices, W.MESH_VERTEX),
                vis=device_array(wptr, (cam.height, cam.width), np.uint64),
                counters=np.array([stats[k] for k in ("skipped", "culled", "per_lane", "cooperative")], np.uint32))


def gpu_arrays(gen, s):
    state, results = gen.bodies_state(s), gen.bodies_results(s)   # both synchronise
    b, _, p = gen.bodies_device_ptrs(s)
    return {"state": state.tobytes(), "records": device_read(b, s.num_bodies, W.BUOYANCY_BODY).tobytes(), "results": results.tobytes(),
            "points": device_read(p, s.num_points, W.BUOYANCY_POINT).tobytes()}


SHADE_KEYS = ("water_color", "foam_color", "roughness", "normal_strength", "light_direction", "light_color", "ambient_color", "sky_color")


DEFAULTS = dict(water_color=(0.0100228256, 0.019606648, 0.0272117816), foam_color=(0.491905034, 0.406448305, 0.34239164), roughness=0.65,
                normal_strength=1.0, light_direction=(0.321197, 0.18296, 0.929171), light_color=(1.0, 1.0, 1.0),
                ambient_color=(0.05, 0.08, 0.10), sky_color=(0.25, 0.40, 0.60))


SUN_LOW = (0.321197, 0.18296, 0.929171)      # main.tscn:113: 10.5 degrees above the horizon, ahead of a camera that looks towards +z


SUN_BEHIND = (0.2, 0.5, -0.84)               # behind that camera


def look(position, yaw_deg, pitch_deg, fov=75.0, width=20, height=12, max_distance=4000.0):
    """an ow_camera at `position` looking along yaw (0 = +z, towards +x as it grows) and pitch (degrees, negative = down), +Y up: the
    basis columns are right, up and back, written as Godot's rows"""
    yaw, pitch = math.radians(yaw_deg), math.radians(pitch_deg)
    f = np.array([math.sin(yaw) * math.cos(pitch), math.sin(pitch), math.cos(yaw) * math.cos(pitch)])
    right = np.cross(f, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, f)
    return W.camera(position, np.stack([right, up, -f], axis=1), fov, width, height, max_distance)


def camera_words(cam):
    """the 15 floats the runtime resolves from an ow_camera: position, basis, tan(fov / 2) in FP64 narrowed, aspect, max_distance"""
    th = np.float32(math.tan(float(cam.fov_y_degrees) * (3.14159265358979323846 / 360.0)))
    aspect = np.float32(cam.width) / np.float32(cam.height)
    return np.array(list(cam.position) + list(cam.basis) + [th, aspect, cam.max_distance], np.float32)


def shade_words(options):
    """the 22 floats of ow::ShadeParams as the runtime resolves them from ow_render_options (the uniform-only constants in FP64)"""
    o = dict(DEFAULTS, **{k: v for k, v in (options or {}).items() if k in SHADE_KEYS})
    f32 = lambda v: [float(np.float32(x)) for x in v]   # noqa: E731
    r = float(np.float32(o["roughness"]))
    lx, ly, lz = f32(o["light_direction"])
    ln = math.sqrt(lx * lx + ly * ly + lz * lz)
    words = f32(o["water_color"]) + f32(o["foam_color"]) + [r, o["normal_strength"], 5.0 * math.exp(-2.69 * r), 1.0 + 22.7 * math.pow(r, 1.5)]
    words += [lx / ln, ly / ln, lz / ln] + f32(o["light_color"]) + f32(o["ambient_color"]) + f32(o["sky_color"])
    return np.array(words, np.float32)


def uniforms_of(options):
    """what the twin is given: the FP32 values of the options"""
    o = dict(DEFAULTS, **{k: v for k, v in (options or {}).items() if k in SHADE_KEYS})
    return {k: (np.float32(v).astype(np.float64) if np.ndim(v) == 0 else np.asarray(v, np.float32).astype(np.float64)) for k, v in o.items()}


def ray_options(options, cam):
    """the ray cast's share of render options, as W.render_options splits them ("falloff": True = around the camera)"""
    o = {k: v for k, v in (options or {}).items() if k not in SHADE_KEYS and k != "falloff"}
    if (options or {}).get("falloff") and o.get("falloff_center") is None:
        o["falloff_center"] = (cam.position[0], cam.position[2])
    return o


def pixel_rays(L, cam):
    cw = camera_words(cam)
    rays = np.zeros(cam.width * cam.height, W.RAY)
    L.harness_pixel_rays(cw.ctypes.data, cam.width, cam.height, rays.ctypes.data)
    return rays


GPU_CAM = dict(position=(0.0, 10.0, -25.0), yaw_deg=5.0, pitch_deg=-10.0)


GROW_SIZES = ((8, 8), (40, 24), (8, 8))   # the scratch is sized exactly: the second image replaces both blocks, the third fits what is there


def render_outputs(gen, cam, sc, rgba=True, pixels=True):
    """ow_render_view with either output left out (the wrapper always asks for the RGBA words)"""
    sc = np.ascontiguousarray(sc, np.float32).reshape(-1, 4)
    o = gen.render_options(None, cam)
    img = np.zeros((cam.height, cam.width, 4), np.uint8) if rgba else None
    rec = np.zeros((cam.height, cam.width), W.RENDER_PIXEL) if pixels else None
    _lib.check(gen._lib.ow_render_view(gen.context, C.byref(cam), sc.ctypes.data, len(sc), C.byref(o) if o is not None else None,
                                       img.ctypes.data if rgba else None, rec.ctypes.data if pixels else None))
    return img, rec


REF_BASIS = (-0.996195, -0.0151344, 0.0858316, 0.0, 0.984807, 0.173648, -0.0871557, 0.172987, -0.981061)   # main.tscn:120


def grid(cells=16, cell=4.0, y=0.0):
    """(cells + 1)^2 vertices around the origin, two triangles a cell, counter-clockwise seen from above"""
    half = 0.5 * cells * cell
    c = np.arange(cells + 1, dtype=np.float32) * np.float32(cell) - np.float32(half)
    x, z = np.meshgrid(c, c)
    v = np.stack([x.ravel(), np.full(x.size, y, np.float32), z.ravel()], axis=1).astype(np.float32)
    r, q = np.meshgrid(np.arange(cells), np.arange(cells), indexing="ij")
    a = (r * (cells + 1) + q).ravel()
    b, d, e = a + 1, a + cells + 1, a + cells + 2
    t = np.stack([np.stack([a, d, b], 1), np.stack([b, d, e], 1)], 1).reshape(-1, 3).astype(np.int32)
    return v, t


def grid_with_a_fan():
    """the 17 x 17 grid with one cell drawn as a pentagon: an extra vertex in the middle of an edge, fanned from the cell's first corner, so
    that one of its triangles has zero area and its neighbour keeps the long edge (a T-junction, as at the clipmap's ring transitions)"""
    v, t = grid()
    cell = 8 * 16 + 5
    a, d, b = t[2 * cell]
    e = t[2 * cell + 1][2]
    mid = len(v)
    v = np.concatenate([v, [(v[a] + v[d]) / 2]]).astype(np.float32)
    fan = np.array([(a, mid, d), (a, d, e), (a, e, b), (a, a, mid)], np.int32)   # (a, mid, d) is collinear; (a, a, mid) has two equal corners
    return v, np.concatenate([t[:2 * cell], t[2 * cell + 2:], fan]).astype(np.int32)


CALM_CAMERAS = {
    "down": (dict(position=(1.0, 20.0, -2.0), yaw_deg=0.0, pitch_deg=-89.9, max_distance=200.0), {}),
    "pitched": (dict(position=(0.0, 12.0, -20.0), yaw_deg=10.0, pitch_deg=-25.0, max_distance=40.0), {}),
    "near_plane": (dict(position=(0.3, 0.5, 0.2), yaw_deg=30.0, pitch_deg=0.0, max_distance=200.0), {}),
    "near_plane_far_cut": (dict(position=(0.3, 0.5, 0.2), yaw_deg=30.0, pitch_deg=0.0, max_distance=25.0), {"near": 3.0}),
}


NO_TRIANGLE = np.uint64(0xFFFFFFFFFFFFFFFF)   # a visibility word no triangle has written


NEAR = 0.05                                  # ow_mesh_options_default's near plane, metres


def center_of(options, cam):
    o = options or {}
    if o.get("falloff_center") is not None:
        return tuple(o["falloff_center"])
    return (cam.position[0], cam.position[2]) if o.get("falloff") and cam is not None else None


SPRAY_DELTA = 1.0 / 50.0


def spray_options(amount, **kw):
    o = _lib.ow_spray_options()
    C.memset(C.byref(o), 0, C.sizeof(o))
    d = dict(amount=amount, emitter_lifetime=6.0, lifetime=3.0, lifetime_randomness=0.25, particle_scale=(20.0, 8.5, 20.0), random_seed=0,
             emission_transform=(15, 0, 0, -1, 0, 15, 0, 0, 0, 0, 15, -25), start_time=0.0, num_particles=0)
    d.update(kw)
    for k, v in d.items():
        if k in ("particle_scale", "emission_transform"):
            getattr(o, k)[:] = [float(x) for x in v]
        else:
            setattr(o, k, v)
    return o


FOAM = DEFAULTS["foam_color"]


MAX_ALPHA = 0.666


def gradient_texture(h=16, w=24):
    """an albedo whose colour differs at every texel and whose alpha is a soft blob that stays above a third"""
    j, i = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    t = np.zeros((h, w, 4), np.uint8)
    t[..., 0] = 40 + 200 * i // max(w - 1, 1)
    t[..., 1] = 250 - 190 * j // max(h - 1, 1)
    t[..., 2] = 60 + (37 * i + 91 * j) % 190
    r2 = ((i + 0.5) / w - 0.5) ** 2 + ((j + 0.5) / h - 0.5) ** 2
    t[..., 3] = np.clip(255 * (1.0 - 1.3 * r2), 90, 255).astype(np.uint8)
    return t


def noise_texture(h=32, w=32, seed=3, hi=140):
    """a dissolve texture: smooth noise in the red channel, low enough that (w + z) / 2 clears it for most particles"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 1, (h, w))
    for _ in range(2):
        a = (a + np.roll(a, 1, 0) + np.roll(a, 1, 1) + np.roll(a, -1, 0) + np.roll(a, -1, 1)) / 5.0
    a = (a - a.min()) / (a.max() - a.min())
    t = np.zeros((h, w, 4), np.uint8)
    t[..., 0] = (a * hi).astype(np.uint8)
    t[..., 1] = 255 - t[..., 0]
    t[..., 3] = 255
    return t


def flat_texture(rgba, h=1, w=1):
    return np.broadcast_to(np.asarray(rgba, np.uint8), (h, w, 4)).copy()


def material(albedo=None, dissolve=None, **kw):
    m = dict(foam_color=FOAM, max_alpha=MAX_ALPHA, albedo=gradient_texture() if albedo is None else albedo,
             dissolve=noise_texture() if dissolve is None else dissolve, albedo_srgb=1, dissolve_srgb=1)
    m.update(kw)
    return m


WHITE = dict(albedo=flat_texture((255, 255, 255, 255)), dissolve=flat_texture((0, 0, 0, 255)))


def billboards(rows):
    """SPRAY_INSTANCE records from (origin, width, height, custom.z, custom.w): the basis is diag(width, height, 1)"""
    out = np.zeros(len(rows), W.SPRAY_INSTANCE)
    for k, (origin, sx, sy, z, w) in enumerate(rows):
        t = np.zeros((3, 4), np.float32)
        t[0, 0], t[1, 1], t[2, 2] = sx, sy, 1.0
        t[:, 3] = origin
        out["transform"][k] = t.ravel()
        out["custom"][k] = (0.0, 0.0, z, w)
    return out


def level_camera(width=64, height=40, position=(0.0, 0.0, 0.0), fov=90.0, max_distance=4000.0):
    """a camera with the identity basis: it looks down -Z, view space is world space minus the position"""
    return W.camera(position, np.eye(3), fov, width, height, max_distance)


def blank_records(cam, color=(0.1, 0.2, 0.3)):
    rec = np.zeros((cam.height, cam.width), W.RENDER_PIXEL)
    rec["color"] = np.float32(color)
    return rec


def gpu_material(gen, mat):
    return gen.spray_material_create(mat["albedo"], mat["dissolve"], {k: mat[k] for k in ("foam_color", "max_alpha", "albedo_srgb", "dissolve_srgb")})


def bare_context():
    """the smallest context: the billboard draw reads no map"""
    return make_gen(128, [0, 1])[0]


def device_buffers(cam):
    import torch
    count = cam.width * cam.height
    return (torch.zeros((count, 4), dtype=torch.uint8, device="cuda:0"),
            torch.zeros((count, W.RENDER_PIXEL.itemsize), dtype=torch.uint8, device="cuda:0"))


def buffers_to_host(cam, rgba_dev, rec_dev):
    return dict(rgba=rgba_dev.cpu().numpy().reshape(cam.height, cam.width, 4),
                rec=np.frombuffer(rec_dev.cpu().numpy().tobytes(), W.RENDER_PIXEL).reshape(cam.height, cam.width).copy())


def example_textures(size=64):
    """examples/scene.h's scene_textures, integer for integer (tests/test_example_scene.py compares the bytes)"""
    s, lattice = 12345, np.zeros((8, 8), np.int64)
    for j in range(8):
        for i in range(8):
            s = (s * 1664525 + 1013904223) % 2 ** 32
            lattice[j, i] = (s >> 24) & 0xFF
    j, i = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    albedo = np.full((size, size, 4), 255, np.uint8)
    r2 = (2 * i + 1 - size) ** 2 + (2 * j + 1 - size) ** 2
    albedo[..., 3] = np.where(r2 >= size * size, 0, 255 - (255 * r2) // (size * size)).astype(np.uint8)
    cx, cy, fx, fy = i // 8, j // 8, i % 8, j % 8
    top = lattice[cy, cx] * (8 - fx) + lattice[cy, (cx + 1) % 8] * fx
    bot = lattice[(cy + 1) % 8, cx] * (8 - fx) + lattice[(cy + 1) % 8, (cx + 1) % 8] * fx
    dissolve = np.zeros((size, size, 4), np.uint8)
    dissolve[..., 0] = dissolve[..., 1] = dissolve[..., 2] = ((top * (8 - fy) + bot * fy) // 128).astype(np.uint8)
    dissolve[..., 3] = 255
    return albedo, dissolve


SUN = (0.321197, 0.18296, 0.929171)


def cube(side=1.0):
    """8 vertices, 12 triangles, counter-clockwise seen from outside; triangles 2 f and 2 f + 1 are face f (-x, +x, -y, +y, -z, +z)"""
    h = 0.5 * side
    v = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], np.float32)   # index = 4 ix + 2 iy + iz
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    t = np.array([tri for a, b, c, d in quads for tri in ((a, b, c), (a, c, d))], np.int32)
    return v, t


def box(size):
    v, t = cube(1.0)
    return (v * np.float32(size)).astype(np.float32), t


def transform(origin=(0.0, 0.0, 0.0), q=(0.0, 0.0, 0.0, 1.0), scale=1.0):
    """twelve floats: the rotation of unit quaternion q (x, y, z, w) as basis rows, times scale, then the origin"""
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    r = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]) * scale
    return np.concatenate([r.ravel(), np.asarray(origin, np.float64)]).astype(np.float32)


def transforms(rows):
    return np.stack([transform(*r) if not isinstance(r, np.ndarray) else r for r in rows]).astype(np.float32) if len(rows) else np.zeros((0, 12), np.float32)


def tumbled(count, seed=5, x=(-4.7, 4.7), y=(-0.9, 1.6), z=(4.3, 9.7)):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(count):
        q = rng.normal(size=4)
        rows.append(((rng.uniform(*x), rng.uniform(*y), rng.uniform(*z)), q / np.linalg.norm(q)))
    return transforms(rows)


SOLID_TWIN_CAM = dict(position=(0.37, 3.1, -1.3), yaw_deg=4.0, pitch_deg=-14.0, fov=75.0, width=96, height=64, max_distance=500.0)


def eight_crates():
    rng = np.random.default_rng(3)
    items = []
    for k in range(8):
        q = rng.normal(size=4)
        items.append(crate(origin=((k % 4 - 1.5) * 4.0 + 0.3, 0.3, 6.0 + 5.0 * (k // 4)), q=tuple(q / np.linalg.norm(q)), kl=3.0, kq=0.5))
    return make_bodies(items)


CRATE_CAM = dict(position=(0.4, 5.0, -9.0), yaw_deg=2.0, pitch_deg=-17.0, fov=75.0, width=160, height=96, max_distance=2000.0)


CRATE_SHAPE = (2.0, 1.0, 2.0)


def floating_scene(n=128, stream=None, steps=6, broken=None):
    """128^2 x 2 maps, eight tumbling crates stepped behind a tick each (one of them overflowing in its first substep: its fault flag is
    raised and its state frozen where it was created), a 4096-particle emitter stepped with them"""
    gen, params = make_gen(n, [0, 1], stream=stream)
    sc = scales_of(params)
    gen.run(UPDATE_DELTA, params, 20)
    st, hull = eight_crates()
    if broken is not None:
        st["applied_force"][broken], st["mass"][broken] = (0, 1.7e308, 0), 1e-3       # passes the host's checks, is not finite after one substep
    bodies = gen.bodies_create(st, hull)
    spray = gen.spray_create({"amount": 4096, "emitter_lifetime": 0.5, "lifetime": 0.25})
    advance(gen, params, sc, bodies, spray, steps)
    return gen, params, sc, bodies, spray


def advance(gen, params, sc, bodies, spray, steps):
    for _ in range(steps):
        gen.update_all(UPDATE_DELTA, params)
        gen.bodies_step(bodies, sc, 2, UPDATE_DELTA / 2, {"warm_start": True})
        gen.spray_step(spray, UPDATE_DELTA, sc)


def pose_transforms(gen, bodies):
    """the set's resident pose records as [bodies][24] floats: the transform is the first twelve"""
    ptr, _, _ = gen.bodies_device_ptrs(bodies)
    rec = device_read(ptr, bodies.num_bodies, W.BUOYANCY_BODY)
    return np.frombuffer(rec.tobytes(), np.float32).reshape(bodies.num_bodies, 24).copy()


def example_crates():
    """examples/scene.h's scene_crates, operation for operation (tests/test_example_scene.py compares the bytes)"""
    size, rho, per = (2.0, 1.0, 2.0), 1025.0, 4 * 2 * 4
    volume = size[0] * size[1] * size[2]
    mass = 0.5 * rho * volume
    st = np.zeros(36, W.RIGID_BODY)
    hull = np.zeros(36 * per, W.HULL_POINT)
    for b in range(36):
        st[b]["position"] = ((b % 6 - 2.5) * 6.0, 0.3, 10.0 + (b // 6 - 2.5) * 6.0)
        st[b]["orientation"] = (0, 0, 0, 1)
        st[b]["mass"] = mass
        st[b]["inverse_inertia"] = (12.0 / (mass * (size[1] * size[1] + size[2] * size[2])), 12.0 / (mass * (size[0] * size[0] + size[2] * size[2])),
                                    12.0 / (mass * (size[0] * size[0] + size[1] * size[1])))
        st[b]["linear_drag"], st[b]["quadratic_drag"] = 3.0, 0.5
        st[b]["point_offset"], st[b]["point_count"] = b * per, per
        k = b * per
        for i in range(4):
            for j in range(2):
                for l in range(4):
                    hull[k]["local"] = ((i + 0.5) * (size[0] / 4) - size[0] / 2, (j + 0.5) * (size[1] / 2) - size[1] / 2, (l + 0.5) * (size[2] / 4) - size[2] / 2)
                    hull[k]["volume"], hull[k]["half_height"], hull[k]["body"] = volume / per, size[1] / 2 / 2, b
                    k += 1
    return st, hull


def gradient_panorama(w=64, h=32, seed=5):
    """a smooth sky: a vertical gradient, brighter towards one azimuth, a little noise so that no two texels are alike"""
    j, i = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w, 4), np.uint8)
    img[..., 0] = 40 + 150 * j // max(h - 1, 1) + rng.integers(0, 8, (h, w))
    img[..., 1] = 90 + 120 * j // max(h - 1, 1) + 20 * np.abs(2 * i - w) // max(w, 1)
    img[..., 2] = 230 - 100 * j // max(h - 1, 1) + rng.integers(0, 8, (h, w))
    img[..., 3] = 255
    return img


def sky_of(image, srgb=1, energy=1.0):
    return dict(image=np.ascontiguousarray(image, np.uint8), srgb=int(srgb), energy=float(np.float32(energy)))


def f32_options(defaults, opts):
    """the options as the library sees them: every number through FP32"""
    o = dict(defaults, **(opts or {}))
    return {k: (tuple(float(np.float32(x)) for x in v) if isinstance(v, (tuple, list, np.ndarray)) else (int(v) if isinstance(v, (int, np.integer)) else
                                                                                                    float(np.float32(v)))) for k, v in o.items()}


def synthetic_records(cam, seed=1, top=50.0):
    """a record field with everything in it: misses of every status, water hits, hits from below and solids at t from 0 to 1000 m (the
    fog's ends and the values next to them included), colours from 0 to `top`"""
    rng = np.random.default_rng(seed)
    shape = (cam.height, cam.width)
    rec = np.zeros(shape, W.RENDER_PIXEL)
    kind = rng.integers(0, 4, shape)
    miss = rng.choice(np.int32([0, 2, 4, 8]), shape)
    rec["status"] = np.where(kind == 0, miss, np.where(kind == 1, HIT, np.where(kind == 2, HIT | SOLID, HIT | 2)))
    special = np.float32([0.0, 200.0, np.nextafter(np.float32(200), np.float32(0)), np.nextafter(np.float32(200), np.float32(400)), 275.0, 350.0,
                          np.nextafter(np.float32(350), np.float32(0)), np.nextafter(np.float32(350), np.float32(400)), 1000.0, 1e-3])
    t = np.where(rng.random(shape) < 0.25, rng.choice(special, shape), rng.uniform(0.0, 1000.0, shape).astype(np.float32))
    rec["t"] = np.where(kind == 0, 0.0, t)
    scale = np.where(rng.random(shape) < 0.5, 1.0, top)
    rec["color"] = (rng.random(shape + (3,)) * scale[..., None]).astype(np.float32)
    rec["color"][rng.random(shape) < 0.05] = 0.0
    rec["specular"] = rng.random(shape).astype(np.float32)        # neighbours of the fields the pass rewrites: they must not move
    rec["reserved"] = rng.integers(0, 1 << 30, shape + (4,))
    return rec


def rel(got, want):
    """|got - want| relative to max(1, |want|), the largest over the array (0 for an empty one)"""
    want = np.asarray(want, np.float64)
    e = np.abs(np.asarray(got, np.float64) - want) / np.maximum(1.0, np.abs(want))
    return float(e.max()) if e.size else 0.0


def gpu_sky(gen, sky):
    return gen.sky_create(sky["image"], {"srgb": sky["srgb"], "energy": sky["energy"]}) if sky is not None else None


def device_frame(cam, s):
    import torch
    count = cam.width * cam.height
    out = (cam.width // s) * (cam.height // s)
    return (torch.zeros((count, W.RENDER_PIXEL.itemsize), dtype=torch.uint8, device="cuda:0"), torch.zeros((out, 4), dtype=torch.uint8, device="cuda:0"),
            torch.zeros((out, 4), dtype=torch.float32, device="cuda:0"))


def records_of(cam, rec_dev):
    return np.frombuffer(rec_dev.cpu().numpy().tobytes(), W.RENDER_PIXEL).reshape(cam.height, cam.width).copy()


FRAME_CAM = dict(position=(-1.0, 12.0, -60.0), yaw_deg=0.0, pitch_deg=-10.0, fov=75.0, width=64, height=40, max_distance=4000.0)


FRAME_WATER = (18, 4.0)          # a 72 m grid round the camera: it ends at z = -24, in the middle of the emitter's box (z from -32.5 to -17.5), so the


FRAME_SPRAY = {"amount": 4096, "emitter_lifetime": 0.5, "lifetime": 0.25, "particle_scale": (60.0, 25.0, 60.0)}   # three times the scene's billboards


FRAME_SHAPE = (4.0, 2.0, 4.0)    # drawn at the crates' poses: large enough to show from 20 m at 64 x 40


FRAME_ENV = dict(depth_begin=20.0, depth_end=120.0)      # the scene is small: fog that shows inside it


FRAME_PRESENT = dict(downsample=2)


def frame_crates():
    """eight tumbled crates in two rows 18 m and 24 m in front of the camera, on the water"""
    rng = np.random.default_rng(3)
    items = []
    for k in range(8):
        q = rng.normal(size=4)
        items.append(crate(origin=((k % 4 - 1.5) * 4.0 - 1.0, 0.3, -42.0 + 6.0 * (k // 4)), q=tuple(q / np.linalg.norm(q)), kl=3.0, kq=0.5))
    return make_bodies(items)


def frame_scene(n=256, ids=(0, 1, 2), ticks=100, steps=30):
    """256^2 x 3 maps 100 ticks in (foam has built up), eight crates and the emitter stepped 30 times behind a tick each"""
    gen, params = make_gen(n, list(ids))
    sc = scales_of(params)
    gen.run(UPDATE_DELTA, params, ticks)
    bodies = gen.bodies_create(*frame_crates())
    spray = gen.spray_create(FRAME_SPRAY)
    advance(gen, params, sc, bodies, spray, steps)
    return gen, params, sc, bodies, spray


def example_panorama(w=256, h=128):
    """examples/scene.h's scene_panorama, integer for integer (tests/test_example_scene.py compares the bytes)"""
    half = h // 2
    j, i = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    up = j < half
    k = np.where(up, j, h - 1 - j)
    az = (20 * np.abs(2 * i - w)) // w
    img = np.zeros((h, w, 4), np.uint8)
    img[..., 0] = np.where(up, 60 + (150 * k) // (half - 1), 30 + (40 * k) // (half - 1)) + az
    img[..., 1] = np.where(up, 110 + (110 * k) // (half - 1), 50 + (50 * k) // (half - 1)) + az
    img[..., 2] = np.where(up, 200 + (40 * k) // (half - 1), 70 + (60 * k) // (half - 1))
    img[..., 3] = 255
    return img


def gpu_radiance(gen, sky, ropts=None):
    """(the Sky, the Radiance) of a sky_of dict"""
    handle = gpu_sky(gen, sky)
    return handle, gen.radiance_create(handle, ropts)

"""Ray casts against the rendered water (include/ocean_waves.h ow_raycast_surface, ow_raycast_surface_async, ow_group_raycast_surface):
where a ray first meets the height field the water-height query reports (godotoceanwaves_amd/csrc/ow_raycast.h).

CPU: the ABI (header, exports, ctypes, NumPy, C, the harness and C# layouts) and the argument checks without a device; ow_raycast.h compiled
as plain C++ (tests/raycast/raycast_harness.cpp, g++ -ffp-contract=off, the 64 lanes of a round stepped in sequence) held to the analytic
hit on a calm sea, to an FP64 twin on a height-only swell and on the demo scene (tests/raycast_twin.py), to the query's records bit for
bit, to its own slab, and to finite records on awkward rays.  GPU: the device records (one wave per ray) are the CPU build's bit for bit,
the asynchronous form is ordered like ow_query_surface_async, and the group form equals a single context."""
import ctypes as C
import re

import numpy as np
import pytest

import raycast_twin as RT
from godotoceanwaves_amd import _lib, build
from godotoceanwaves_amd.presets import UPDATE_DELTA
from godotoceanwaves_amd.wave_generator import WaveGenerator as W
import checks as S
from checks import check_calm_hits, check_calm_misses, check_csharp_binds, check_declared_and_bound, check_records, exported_symbols, HEADER
from cpu_builds import cpu_raycast, layout_probe
from cpu_builds import query_harness, raycast_harness as harness  # noqa: F401 (fixtures)
from scenes import (BELOW, calm_hit_rays, calm_maps, calm_miss_rays, camera_rays, generated_maps, gpu_maps, HIT, INVALID, make_gen, mixed_rays,
                    RAY_TOL as TOL, scales_of, slope_factor, smallest_context, SPACING, swell_maps, swell_rays, TRUNC, unit)

NEW_FUNCTIONS = ("ow_raycast_surface", "ow_raycast_surface_async", "ow_group_raycast_surface")
STRUCTS = {"OwRay": "ow_ray", "OwRaycastOptions": "ow_raycast_options", "OwRaycastHit": "ow_raycast_hit"}


# ---- 1. the ABI ----------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_ray_cast_and_the_library_exports_it():
    build.build_library()
    lib = _lib.load()
    text = check_declared_and_bound(lib, NEW_FUNCTIONS)
    for struct in STRUCTS.values():
        assert re.search(r"typedef struct %s \{" % struct, text), struct
    for bit, value in (("OW_RAY_HIT", 1), ("OW_RAY_FROM_BELOW", 2), ("OW_RAY_TRUNCATED", 4), ("OW_RAY_INVALID", 8)):
        assert re.search(r"#define %s %d\b" % (bit, value), HEADER) and getattr(_lib, bit) == value
    exported = exported_symbols()
    assert set(NEW_FUNCTIONS) <= exported
    assert len([s for s in exported if "raycast" in s]) == 3
    assert lib.ow_abi_version() == 4


def test_ray_structs_agree_in_c_ctypes_numpy_and_the_harness(tmp_path, harness):
    fields = [("ow_ray", f) for f in ("origin", "max_distance", "direction", "reserved")]
    fields += [("ow_raycast_options", f) for f in ("query", "water_level", "sample_spacing", "tolerance", "max_samples", "reserved")]
    fields += [("ow_raycast_hit", f) for f in ("t", "position", "residual", "status", "samples", "rounds", "slab_half_height", "t_enter",
                                               "t_exit", "reserved", "query")]
    expr = ", ".join(["sizeof(ow_ray)", "sizeof(ow_raycast_options)", "sizeof(ow_raycast_hit)"] + ["offsetof(%s, %s)" % f for f in fields])
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ocean_waves.h"\nint main(void){printf("%s\\n", ' % " ".join(["%zu"] * (3 + len(fields)))
           + expr + ");return 0;}\n")
    got = layout_probe(tmp_path, "ray_layout", src)
    types = {"ow_ray": (_lib.ow_ray, W.RAY), "ow_raycast_options": (_lib.ow_raycast_options, W.RAYCAST_OPTIONS),
             "ow_raycast_hit": (_lib.ow_raycast_hit, W.RAYCAST_HIT)}
    want_ctypes = [C.sizeof(types[s][0]) for s in ("ow_ray", "ow_raycast_options", "ow_raycast_hit")]
    want_ctypes += [getattr(types[s][0], f).offset for s, f in fields]
    want_numpy = [types[s][1].itemsize for s in ("ow_ray", "ow_raycast_options", "ow_raycast_hit")]
    want_numpy += [types[s][1].fields[f][1] for s, f in fields]
    assert got == want_ctypes == want_numpy
    assert got[:3] == [32, 64, 192]
    assert W.RAYCAST_HIT.fields["query"][0] == W.SURFACE_QUERY and W.RAYCAST_OPTIONS.fields["query"][0].itemsize == 32
    sizes = (C.c_int * 6)()
    harness.harness_raycast_sizes(sizes)
    hit = dict((f, o) for (s, f), o in zip(fields, got[3:]) if s == "ow_raycast_hit")
    assert list(sizes) == [32, 192, 16, hit["status"], hit["slab_half_height"], hit["query"]] == [32, 192, 16, 20, 32, 64]


def test_the_csharp_binding_shows_the_ray_structs_and_functions():
    """the three new [StructLayout] structs list the C fields in order with the same sizes (embedded records counted as
    their bytes), the three functions are bound, §7 names them, and the intersect_ray mapping is written down"""
    c_sizes = dict(S.C_SIZES, ow_query_options=32, ow_surface_query=128)
    cs_sizes = dict(S.CS_SIZES, OwQueryOptions=32, OwSurfaceQuery=128)

    def fields(body, sizes, strip):
        out = []
        for decl in body.split(";"):
            decl = " ".join(strip(decl).split())
            if not decl:
                continue
            decl = decl[len("fixed "):] if decl.startswith("fixed ") else decl
            typ, names = decl.split(" ", 1)
            for n in names.split(","):
                m = re.match(r"\s*([A-Za-z_]\w*)(\[(\d+)\])?\s*$", n)
                out.append((m.group(1), sizes[typ] * int(m.group(3) or 1)))
        return out

    for cs, c in STRUCTS.items():
        cbody = re.search(r"typedef struct %s \{(.*?)\}\s*%s\s*;" % (c, c), S.strip_comments(S.HEADER), flags=re.S).group(1)
        csbody = re.search(r"struct %s \{(.*?)\n\}" % cs, S.strip_comments(S.SHIM), flags=re.S).group(1)
        want = fields(cbody, c_sizes, lambda d: d)
        got = fields(csbody, cs_sizes, lambda d: d.replace("public", ""))
        assert got == want, (cs, got, want)
        assert sum(s for _, s in want) == {"ow_ray": 32, "ow_raycast_options": 64, "ow_raycast_hit": 192}[c]
    check_csharp_binds(NEW_FUNCTIONS, returns="int")
    assert "intersect_ray" in S.DOC and "direction = to − from" in S.DOC


# ---- 2. argument checks without a device ---------------------------------------------------------------------------------------------

def test_ray_cast_argument_errors_without_a_device():
    lib = _lib.load()
    rays = np.zeros(4, W.RAY)
    sc = np.ones((1, 4), np.float32)
    out = np.zeros(4, W.RAYCAST_HIT)
    for count, cascades in ((4, 1), (-1, 1), (4, 0), (4, 9)):
        assert lib.ow_raycast_surface(None, rays.ctypes.data, count, sc.ctypes.data, cascades, None, out.ctypes.data) == _lib.OW_ERR_INVALID
        assert lib.ow_raycast_surface_async(None, 0, count, sc.ctypes.data, cascades, None, 0) == _lib.OW_ERR_INVALID
        assert lib.ow_group_raycast_surface(None, rays.ctypes.data, count, sc.ctypes.data, cascades, None, out.ctypes.data) == _lib.OW_ERR_INVALID
    assert b"null" in lib.ow_last_error()
    assert not out.tobytes().strip(b"\0")
    with pytest.raises(ValueError):
        W.raycast_options({"spacing": 1.0})
    o = W.raycast_options({"water_level": 2.0, "sample_spacing": 0.5, "tolerance": 1e-4, "max_samples": 64, "falloff_center": (1.0, 2.0),
                           "query_tolerance": 1e-5})
    assert (o.water_level, o.sample_spacing, o.max_samples, o.query.flags, tuple(o.query.falloff_center_xz)) == (
        2.0, 0.5, 64, _lib.OW_QUERY_DISTANCE_FALLOFF, (1.0, 2.0))
    assert abs(o.tolerance - 1e-4) < 1e-10 and abs(o.query.tolerance - 1e-5) < 1e-12
    r = W.rays([(0, 10, 0)], [(3, -4, 0)], 50.0)
    assert r["max_distance"][0] == 50.0 and list(r["direction"][0]) == [3, -4, 0]


# ---- 3. the CPU build: a calm sea -----------------------------------------------------------------------------------------------------

def test_calm_sea_hits_at_the_analytic_t(harness, query_harness):
    d, m, sc = calm_maps()
    wl = 1.25
    rays, h = calm_hit_rays(wl)
    opts = {"water_level": wl}
    out = cpu_raycast(harness, d, m, sc, rays, opts)
    hit = check_records(harness, query_harness, d, m, sc, rays, out, opts)
    assert hit.all()
    check_calm_hits(out, rays, h)


def test_calm_sea_misses_from_below_and_truncation(harness):
    d, m, sc = calm_maps()
    wl = -0.5
    opts = {"water_level": wl}
    rays = calm_miss_rays(wl)
    out = cpu_raycast(harness, d, m, sc, rays, dict(opts, max_samples=64))
    check_calm_misses(out, wl)
    full = cpu_raycast(harness, d, m, sc, rays[6:7], dict(opts, max_samples=1 << 20))
    assert full["status"][0] == BELOW and full["samples"][0] == 20001   # to t_exit = 5000 m at 0.25 m: not truncated


# ---- 4. the CPU build: a height-only swell against the FP64 twin -------------------------------------------------------------------------

def test_swell_against_the_fp64_twin(harness, query_harness):
    d, m, sc = swell_maps()
    rays = swell_rays()
    out, mh = cpu_raycast(harness, d, m, sc, rays, probe=True)
    hit = check_records(harness, query_harness, d, m, sc, rays, out)
    assert hit.all()
    dn = unit(rays["direction"]).astype(np.float64)
    t_star = RT.raycast(RT.Field(d, sc), rays["origin"].astype(np.float64), dn, out["t_enter"].astype(np.float64),
                        out["t_exit"].astype(np.float64), SPACING / 16)
    err = np.abs(out["t"] - t_star)
    assert np.isfinite(t_star).all() and err.max() <= TOL + 1e-5, err.max()
    k_a = 2 * np.pi / 20.0 * 1.5                                   # the swell's steepest slope
    assert (np.abs(out["residual"]) <= TOL * slope_factor(dn, k_a) + 1e-5).all()
    assert (mh <= out["slab_half_height"]).all() and out["slab_half_height"][0] <= 1.5 * (1 + 2 ** -10) + 0.01 + 1e-6


# ---- 5. the CPU build: the demo scene against the FP64 twin ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def demo_maps():
    return generated_maps(1024, [0, 1, 2])


# name, rays, options, the least share of rays whose t agrees with the twin within 1e-2 m (agreement measured when this was written)
FAMILIES = [
    ("steep", dict(count=80, heights=(2, 300), angles=(30, 80), seed=1), None, 0.80),
    ("moderate", dict(count=40, heights=(2, 300), angles=(10, 30), seed=2), None, 0.70),
    ("grazing", dict(count=40, heights=(2, 10), angles=(2, 10), seed=3), None, 0.55),
    ("falloff", dict(count=80, heights=(2, 300), angles=(2, 80), seed=4), {"falloff_center": (0.0, 0.0)}, 0.85),
]


@pytest.mark.parametrize("name,rays,options,least", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_demo_scene_against_the_fp64_twin(harness, query_harness, demo_maps, name, rays, options, least):
    """Camera rays over cascades 0-2 of the demo scene at 1024^2.  The twin samples from t_enter at spacing / 16 in FP64 and bisects the
    first change; it is run up to one spacing past the CPU build's hit (a crossing the build missed lies before it).  The rays that
    disagree sit on folded crests (the record's query did not converge, or the cold solve switches sheets between samples, which makes g
    jump) or on crests thinner than the spacing along the ray; grazing rays meet most of both."""
    d, m, sc = demo_maps
    r = camera_rays(**rays)
    out, mh = cpu_raycast(harness, d, m, sc, r, options, probe=True)
    hit = check_records(harness, query_harness, d, m, sc, r, out, options)
    assert (mh <= out["slab_half_height"]).all()
    dn = unit(r["direction"]).astype(np.float64)
    t_end = np.where(hit, np.minimum(out["t"] + SPACING, out["t_exit"]), out["t_exit"]).astype(np.float64)
    center = (options or {}).get("falloff_center")
    t_star = RT.raycast(RT.Field(d, sc, center), r["origin"].astype(np.float64), dn, out["t_enter"].astype(np.float64), t_end, SPACING / 16)
    err = np.abs(out["t"] - t_star)
    agree = hit & np.isfinite(t_star) & (err <= 1e-2)
    conv = out["query"]["converged"] == 1
    print(f"{name}: hits {hit.mean():.3f}, agree {agree.mean():.3f} (converged hits {agree[conv].mean():.3f}), median |t - t*| "
          f"{np.median(err[agree]):.1e} m, {out['samples'].mean():.0f} samples and {out['rounds'].mean():.2f} rounds per ray")
    assert agree.mean() >= least
    assert np.median(err[agree]) <= TOL


# ---- 6. no NaN or Inf on awkward rays ------------------------------------------------------------------------------------------------

def test_no_nan_or_inf_on_awkward_rays(harness, query_harness, demo_maps):
    d, m, sc = demo_maps
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    hw = cpu_raycast(harness, d, m, sc, W.rays([(0, 50, 0)], [(0, -1, 0)], 100.0))["slab_half_height"][0]
    bad = W.rays([(nan, 10, 0), (0, inf, 0), (0, 10, 0), (0, 10, 0), (0, 10, 0), (0, 10, 0), (0, 10, 0), (0, 10, 0), (0, 10, 0)],
                 [(0, -1, 0), (0, -1, 0), (nan, -1, 0), (0, -inf, 0), (0, 0, 0), (1e-30, 0, 0), (3e38, -3e38, 0), (0, -1, 0), (0, -1, 0)],
                 [100, 100, 100, 100, 100, 100, 100, inf, 0.0])
    bad["max_distance"][8] = -5.0
    out = cpu_raycast(harness, d, m, sc, bad)
    assert (out["status"] == INVALID).all() and not out.tobytes().replace(np.int32(INVALID).tobytes(), b"").strip(b"\0")
    odd = W.rays([(0, 30, 0), (5, 30, 7), (0, hw, 0), (0, -hw, 0), (0, 2, 0), (1e4, 3, -1e4), (0, 0.5, 0), (0, 40, 0)],
                 [(0, -1, 0), (0, -1e-3, 0), (1, 0, 0), (1, 0, 0), (1, -1e-6, 1), (-1, -0.05, 1), (1, 0, 0), (0.3, -1, 0.2)],
                 [1e30, 1e30, 1e3, 1e3, 1e30, 1e30, 1e30, 3e38])
    for options in (None, {"falloff_center": (0.0, 0.0), "max_samples": 1000}, {"water_level": -1e3}, {"sample_spacing": 1.0, "tolerance": 0.1}):
        out, mh = cpu_raycast(harness, d, m, sc, odd, options, probe=True)
        check_records(harness, query_harness, d, m, sc, odd, out, options)
        assert not (out["status"] & INVALID).any() and (mh <= out["slab_half_height"]).all()
        assert np.isfinite(out["query"]["height"]).all() and np.isfinite(out["query"]["residual"]).all()


# ---- 7-10. on the GPU ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n,ids", [(1024, [0, 1, 2]), (256, [0, 1, 2, 3]), (2048, [0])])
def test_gpu_records_are_the_cpu_builds_bit_for_bit(harness, n, ids):
    gen, params = make_gen(n, ids)
    gen.run(UPDATE_DELTA, params, 3)
    sc = scales_of(params)
    d, m = gpu_maps(gen, len(ids))
    rays = mixed_rays(n)
    for opts in (None, {"falloff_center": (12.5, -40.0)}, {"water_level": 0.7, "max_samples": 200, "sample_spacing": 0.5}):
        got = gen.raycast_surface(rays, sc, opts)
        want = cpu_raycast(harness, d, m, sc, rays, opts)
        for f in W.RAYCAST_HIT.names:
            assert got[f].tobytes() == want[f].tobytes(), (opts, f)
        st = got["status"]
        assert ((st & HIT) != 0).mean() > 0.5 and ((st & INVALID) != 0).sum() == 2
    assert ((got["status"] & TRUNC) != 0).any()   # the last options: 200 samples -- grazing rays run out


def _async_case(drive, stream=None, torch_stream=None):
    """drive(gen, params, 8) / raycast_surface_async / drive again / sync, against the synchronous ray cast of a context that stopped after
    the first drive: the asynchronous cast read the maps of exactly that point of the stream"""
    import torch
    n, ids = 1024, [0, 1, 2, 3]
    a, pa = make_gen(n, ids, stream=stream)
    b, pb = make_gen(n, ids)
    sc = scales_of(pa)
    rays = mixed_rays(7)
    rays_dev = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda:0")
    out_dev = torch.zeros((len(rays), W.RAYCAST_HIT.itemsize), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    drive(a, pa, 8)
    if torch_stream is not None:
        with torch.cuda.stream(torch_stream):
            a.raycast_surface_async(rays_dev, sc, out_dev)
            copy = out_dev.to("cpu", non_blocking=False)   # the caller's own work, ordered by its stream alone
        torch_stream.synchronize()
    else:
        a.raycast_surface_async(rays_dev, sc, out_dev)
    drive(a, pa, 8)
    a.sync()
    got = np.frombuffer(out_dev.cpu().numpy().tobytes(), W.RAYCAST_HIT)
    drive(b, pb, 8)
    want = b.raycast_surface(rays, sc)
    assert got.tobytes() == want.tobytes()
    if torch_stream is not None:
        assert np.frombuffer(copy.numpy().tobytes(), W.RAYCAST_HIT).tobytes() == want.tobytes()
    # ... and the second half moved the maps: a cast now reads other bits
    assert a.raycast_surface(rays[:500], sc).tobytes() != want[:500].tobytes()
    return a


@pytest.mark.gpu
def test_async_ray_cast_is_ordered_behind_both_chains_on_the_contexts_stream():
    a = _async_case(lambda g, p, k: g.run(UPDATE_DELTA, p, k))
    assert a.chain_stats() > 0


@pytest.mark.gpu
def test_async_ray_cast_on_a_callers_stream():
    import torch
    s = torch.cuda.Stream()
    _async_case(lambda g, p, k: g.run(UPDATE_DELTA, p, k), stream=s.cuda_stream, torch_stream=s)


@pytest.mark.gpu
def test_async_ray_cast_between_look_ahead_ticks():
    def ticks(g, p, k):
        for _ in range(k):
            g.update_all(UPDATE_DELTA, p)
    a = _async_case(ticks)
    hits, _ = a.lookahead_stats()
    assert hits > 0


@pytest.mark.gpu
def test_async_ray_cast_argument_errors():
    import torch
    gen, params = make_gen(256, [0, 1])
    sc = scales_of(params)
    rays_dev = torch.zeros((8, W.RAY.itemsize), dtype=torch.uint8, device="cuda:0")
    out_dev = torch.zeros((8, W.RAYCAST_HIT.itemsize), dtype=torch.uint8, device="cuda:0")
    reserved = _lib.ow_raycast_options()
    reserved.reserved[2] = 1
    for bad in ({"max_samples": -1}, {"max_samples": (1 << 20) + 1}, {"tolerance": float("nan")}, {"sample_spacing": float("inf")},
                {"water_level": float("nan")}, {"max_iterations": 65}, {"falloff_center": (float("inf"), 0.0)}, reserved):
        with pytest.raises(_lib.OceanWavesError) as e:
            gen.raycast_surface_async(rays_dev, sc, out_dev, bad)
        assert e.value.status == _lib.OW_ERR_INVALID
        with pytest.raises(_lib.OceanWavesError):
            gen.raycast_surface(np.zeros(8, W.RAY), sc, bad)
    with pytest.raises(_lib.OceanWavesError) as e:
        gen.raycast_surface(np.zeros(8, W.RAY), np.ones((3, 4), np.float32))
    assert e.value.status == _lib.OW_ERR_INVALID
    with pytest.raises(ValueError):
        gen.raycast_surface_async(rays_dev, sc, out_dev[:4])
    assert len(gen.raycast_surface(np.zeros(0, W.RAY), sc)) == 0
    torch.cuda.synchronize()
    assert not out_dev.any()


@pytest.mark.gpu
def test_group_ray_cast_equals_a_single_context():
    from godotoceanwaves_amd import WaveCascadeParameters, WaveGeneratorGroup
    from godotoceanwaves_amd.presets import cascade_preset
    n, ids = 512, [0, 1, 2, 3]
    grp = WaveGeneratorGroup()
    grp.map_size = n
    grp.init_gpu([0, 0], 2)
    pg = [WaveCascadeParameters(**cascade_preset(ci)) for ci in ids]
    single, ps = make_gen(n, ids)
    rays = mixed_rays(3)
    sc = scales_of(ps)
    with pytest.raises(_lib.OceanWavesError) as e:   # nothing gathered yet
        grp.raycast_surface(rays, sc)
    assert e.value.status == _lib.OW_ERR_STATE
    grp.run(UPDATE_DELTA, pg, 4)
    single.run(UPDATE_DELTA, ps, 4)
    grp.gather_begin()
    grp.gather_wait()
    for opts in (None, {"falloff_center": (-30.0, 60.0), "water_level": 0.25}):
        assert grp.raycast_surface(rays, sc, opts).tobytes() == single.raycast_surface(rays, sc, opts).tobytes()


@pytest.mark.gpu
def test_ray_scratch_grows_past_its_floor_and_stays(harness):
    """8 rays, 1 025 (one past the scratch's floor of 1 024: the block is replaced), 8 again on one context: the CPU build's records each time"""
    gen, sc, d, m = smallest_context()
    for k, count in enumerate((8, 1025, 8)):
        rays = camera_rays(count, (2, 300), (2, 80), seed=50 + k)
        got, want = gen.raycast_surface(rays, sc), cpu_raycast(harness, d, m, sc, rays)
        for f in W.RAYCAST_HIT.names:
            assert got[f].tobytes() == want[f].tobytes(), (count, f)
        assert ((got["status"] & HIT) != 0).any(), count
    gen.free()

"""The floating bodies reflected in the water (include/ocean_waves.h ow_mirror_*, godotoceanwaves_amd/csrc/ow_mirror.h).

CPU: the ABI, the documents and every refusal without a device; ow_mirror.h compiled as plain C++ (tests/mirror/mirror_harness.cpp, g++
-ffp-contract=off) held to its bit identities (no bodies is the sky pass; the hit is the cast's; culling does not show; twice is once;
after the sky pass, nothing), to an FP64 twin written from the definition (tests/mirror_twin.py; the observed figures are in
profiles/mirror_margins.txt), to the closed form of one box over a flat sea and to the fade's two ends; the kernel's tile cull drops no
instance a lane would have passed.  GPU: k_mirror_apply is the CPU build's bit for bit -- records, hits and counters -- on hand-built records of every kind at the chunk edges of the
instance count and on a drawn sea with crates; every form of the call gives the same bytes; examples/mirror_host.c writes a frame whose
water, and only whose water, differs from the sky pass's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mirror_twin as MT
import sky_light_twin as SL
from godotoceanwaves_amd import _lib, build, mirror, solid_cast as SC
from godotoceanwaves_amd.wave_generator import WaveGenerator as W
import checks as S
from checks import check_declared_and_bound, exported_symbols, HEADER
from cpu_builds import build_example, CpuPyramid, CSRC, harness_library, layout_probe, RADIANCE_DEFAULTS, ROOT
from cpu_builds import sky_harness  # noqa: F401 (fixture)
from helpers import TOL_F32
from scenes import (bare_context, box, camera_words, crate, device_buffers, frame_scene, FRAME_SHAPE, FRAME_WATER, gpu_radiance, gradient_panorama, grid, HIT,
                    level_camera, look, make_bodies, pose_transforms, records_of, rel, sky_of, transform, transforms)

MARGINS = os.path.join(ROOT, "profiles", "mirror_margins.txt")
NEW_FUNCTIONS = ("ow_mirror_options_init", "ow_mirror_apply", "ow_mirror_apply_async", "ow_mirror_apply_instances", "ow_mirror_stats")
BELOW, INVALID, SOLID, ENV, LIT, MIRROR = (_lib.OW_RAY_FROM_BELOW, _lib.OW_RAY_INVALID, _lib.OW_RAY_SOLID, _lib.OW_RAY_ENVIRONMENT, _lib.OW_RAY_SKY_LIT,
                                            _lib.OW_RAY_MIRROR)
CASE = np.dtype([("width", np.int32), ("height", np.int32), ("cam", np.float32, 15), ("num_vertices", np.int32), ("num_triangles", np.int32),
                 ("count", np.int32), ("stride", np.int32), ("has_flags", np.int32), ("options", np.uint8, 128)])
STAGES = (("view", 0, 3), ("reflect", 3, 6), ("lod", 6, 7), ("radiance", 7, 10), ("env", 10, 12), ("irradiance", 12, 15), ("ambient", 15, 18), ("spec", 18, 21),
          ("body", 21, 24), ("weight", 24, 25), ("cast", 25, 26))
COUNTERS = ("pixels", "rays_cast", "sphere_tests_passed", "pairs_tested", "rays_hit")
ROPTS = dict(levels=4, samples=16)          # a 64 x 32 sky has four levels
PICTURES = ((21, 13), (24, 16))             # partial tiles on both sides, and exact tiles
COUNTS = (0, 1, 63, 64, 65, 130)            # the chunk edges of the instance loop
f32 = np.float32


# ---- shapes, records and the CPU build -----------------------------------------------------------------------------------------------------

def one_triangle():
    """a single triangle that faces down: what a mirror ray, which rises, meets from the front"""
    return np.float32([(-1.5, 0, -1.5), (1.5, 0, -1.5), (0, 0, 1.5)]), np.int32([(0, 1, 2)])


def fan(n=65, radius=1.5):
    """n triangles round a centre, facing down"""
    a = 2 * np.pi * np.arange(n) / n
    v = np.concatenate([[(0.0, 0.0, 0.0)], np.stack([radius * np.cos(a), np.zeros(n), radius * np.sin(a)], 1)]).astype(np.float32)
    return v, np.int32([(0, 1 + k, 1 + (k + 1) % n) for k in range(n)])


SHAPES = {1: one_triangle(), 12: box((2.0, 1.0, 2.0)), 65: fan()}


def view_camera(w, h):
    return look(position=(0.3, 3.0, -2.0), yaw_deg=3.0, pitch_deg=-14.0, fov=75.0, width=w, height=h, max_distance=4000.0)


def sea_records(cam, seed=1, ripple=0.03, kinds=True, far=False):
    """Hand-built records: a sea on y = 0 under the camera's pixel rays (rippled unit normals about +Y, roughness over [0, 0.5]), the sky above
    the horizon, and with `kinds` one or more records of every other kind among the water: a solid, water seen from below, records that
    carry OW_RAY_ENVIRONMENT or OW_RAY_SKY_LIT already, a zero normal, normals that are not finite and roughness outside [0, 1]; with `far`
    two positions 1e30 m away as well (the squared distance overflows in FP32: V and R are zero and the mirror ray is invalid)"""
    rng = np.random.default_rng(seed)
    h, w = cam.height, cam.width
    words = np.asarray(camera_words(cam), np.float64)
    rays = SL.ET.rays(words, w, h)
    down = rays[..., 1] < -1e-3
    t = np.where(down, -words[1] / np.where(down, rays[..., 1], -1.0), 0.0)
    rec = np.zeros((h, w), W.RENDER_PIXEL)
    rec["status"] = np.where(down, HIT, 0)
    rec["t"] = t
    pos = words[0:3] + rays * t[..., None]
    pos[..., 1] = 0.0
    rec["position"] = np.where(down[..., None], pos, 0.0)
    n = np.stack([rng.normal(0, ripple, (h, w)), np.ones((h, w)), rng.normal(0, ripple, (h, w))], -1)
    rec["normal"] = np.where(down[..., None], n / np.linalg.norm(n, axis=-1, keepdims=True), 0.0)
    rec["albedo"] = rng.random((h, w, 3)) * 0.2
    rec["roughness"] = rng.random((h, w)) * 0.5
    rec["color"] = rng.random((h, w, 3)) * 0.1
    rec["specular"], rec["fresnel"] = rng.random((h, w)), rng.random((h, w))       # neighbours of what the pass reads and writes: they must not move
    rec["reserved"] = rng.integers(0, 1 << 30, (h, w, 4))
    if kinds:
        at = np.argwhere(down)
        pick = at[rng.choice(len(at), 16, replace=False)]
        nan, inf = np.nan, np.inf
        for k, (j, i) in enumerate(pick):
            r = rec[j, i:i + 1]
            if k < 2:
                r["status"] = HIT | SOLID
            elif k < 4:
                r["status"] = HIT | BELOW
            elif k < 6:
                r["status"] = HIT | ENV
            elif k < 8:
                r["status"] = HIT | LIT
            elif k < 10:
                r["normal"] = (0.0, 0.0, 0.0)
            elif k < 12:
                r["normal"] = (nan, 1.0, 0.0) if k == 10 else (0.0, inf, 0.0)
            elif k < 14:
                if far:
                    r["position"] = (1e30, 0.0, 5.0) if k == 12 else (1.0, 0.0, -2e30)
            else:
                r["roughness"] = nan if k == 14 else 2.0
    return rec


def crates_over(count, seed=11, x=(-9.0, 9.0), y=(0.3, 2.6), z=(2.0, 34.0)):
    """`count` tumbled instances over the sea in front of view_camera, the middle one (where there are three or more) with a transform that
    is not finite: it is skipped"""
    rng = np.random.default_rng(seed + count)
    rows = []
    for _ in range(count):
        q = rng.normal(size=4)
        rows.append(((rng.uniform(*x), rng.uniform(*y), rng.uniform(*z)), q / np.linalg.norm(q), rng.uniform(0.7, 1.6)))
    tf = transforms(rows)
    if count >= 3:
        tf[count // 2, 4] = np.nan
    return tf


@pytest.fixture(scope="module")
def harness():
    L = harness_library("mirror")
    V = C.c_void_p
    L.harness_mirror_sizes.argtypes = [V]
    L.harness_mirror_apply.argtypes = [V] * 10
    L.harness_radiance_new.argtypes = [V, V]
    L.harness_radiance_new.restype = V
    L.harness_radiance_free.argtypes = [V]
    return L


PANO = sky_of(gradient_panorama(), 1, 1.0)


class MirrorPyramid:
    """the pyramid inside the mirror harness's own library (it includes the sky-light harness): the same CPU build, another load address"""

    def __init__(self, L, sky=PANO, opts=ROPTS):
        o = dict(RADIANCE_DEFAULTS, **opts)
        case = np.zeros(1, np.dtype([("sky_width", np.int32), ("sky_height", np.int32), ("sky_srgb", np.int32), ("energy", np.float32), ("levels", np.int32),
                                     ("samples", np.int32), ("base_width", np.int32)]))
        case["sky_height"], case["sky_width"], case["sky_srgb"], case["energy"] = sky["image"].shape[0], sky["image"].shape[1], sky["srgb"], sky["energy"]
        case["levels"], case["samples"], case["base_width"] = o["levels"], o["samples"], o["base_width"]
        self.L = L
        self.ptr = L.harness_radiance_new(case.ctypes.data, sky["image"].ctypes.data)
        assert self.ptr

    def __del__(self):
        if getattr(self, "ptr", None):
            self.L.harness_radiance_free(self.ptr)


@pytest.fixture(scope="module")
def pyramid(harness):
    return MirrorPyramid(harness)


@pytest.fixture(scope="module")
def sky_pyramid(sky_harness):   # noqa: F811
    """the sky-light harness's pyramid of the same sky: what ow_radiance_light_apply's CPU build works on"""
    return CpuPyramid(sky_harness, PANO, ROPTS)


def options_of(opts=None):
    o = mirror.mirror_options(opts)
    if o is None:
        o = _lib.ow_mirror_options()
        _lib.load().ow_mirror_options_init(C.byref(o))
    return o


def values_of(o):
    """the option record as the twin reads it"""
    v = {k: (tuple(getattr(o, k)) if isinstance(getattr(o, k), C.Array) else getattr(o, k)) for k, _ in o._fields_ if k != "reserved"}
    v["two_sided"] = bool(o.flags & _lib.OW_MIRROR_TWO_SIDED)
    return v


def light_options(o):
    return dict(ambient_energy=o.ambient_energy, reflection_energy=o.reflection_energy, specular=o.specular)


def cpu_mirror(L, pyr, cam, records, shape=None, tf=None, opts=None, stride=12, flags=None):
    """the CPU build's pass: dict of rec (a copy, rewritten), hits, the counters (skipped and COUNTERS) and the stages"""
    rec = np.array(records, W.RENDER_PIXEL, copy=True, order="C")
    assert rec.shape == (cam.height, cam.width)
    o = options_of(opts)
    v = np.ascontiguousarray(shape[0], np.float32).reshape(-1, 3) if shape is not None else np.zeros((0, 3), np.float32)
    t = np.ascontiguousarray(shape[1], np.int32).reshape(-1, 3) if shape is not None else np.zeros((0, 3), np.int32)
    tf = np.ascontiguousarray(tf if tf is not None else [], np.float32).reshape(-1)
    fl = np.ascontiguousarray(flags, np.int32) if flags is not None else None
    h = np.zeros(1, CASE)
    h["width"], h["height"], h["cam"] = cam.width, cam.height, camera_words(cam)
    h["num_vertices"], h["num_triangles"], h["count"], h["stride"], h["has_flags"] = len(v), len(t), tf.size // stride, stride, int(fl is not None)
    h["options"] = np.frombuffer(bytes(o), np.uint8)
    hits = np.zeros(rec.shape, SC.SOLID_HIT)
    counters = np.zeros(9, np.uint64)
    st = np.zeros(rec.shape + (26,), np.float32)
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None    # noqa: E731
    L.harness_mirror_apply(pyr.ptr, h.ctypes.data, ptr(v), ptr(t), ptr(tf), ptr(fl), rec.ctypes.data, hits.ctypes.data, counters.ctypes.data, st.ctypes.data)
    out = dict(rec=rec, hits=hits, skipped=int(counters[0]), **{k: int(counters[1 + i]) for i, k in enumerate(COUNTERS)})
    out.update(cull_tested=int(counters[6]), cull_dropped=int(counters[7]), cull_mistakes=int(counters[8]))   # the kernel's tile cull, checked on the way
    for name, a, b in STAGES:
        out[name] = st[..., a] if b == a + 1 else st[..., a:b]
    out["cast"] = out["cast"] != 0
    return out


def no_hit_records(shape):
    h = np.zeros(shape, SC.SOLID_HIT)
    h["instance"] = h["triangle"] = -1
    return h


def same_records(got, want, what=""):
    for f in W.RENDER_PIXEL.names:
        assert got[f].tobytes() == want[f].tobytes(), (what, f)


def margins():
    out = {}
    for line in open(MARGINS):
        m = re.match(r"margin (\w+) ([0-9.e+-]+)", line)
        if m:
            out[m.group(1)] = float(m.group(2))
    return out


# ---- 1. the interface and the documents -----------------------------------------------------------------------------------------------------

def test_header_declares_the_new_calls_and_the_library_exports_them():
    build.build_library()
    lib = _lib.load()
    check_declared_and_bound(lib, NEW_FUNCTIONS)
    assert sorted(s for s in exported_symbols() if "mirror" in s) == sorted(NEW_FUNCTIONS)      # no group form, no handle: no create, no destroy
    for define, value in (("OW_RAY_MIRROR", "512"), ("OW_MIRROR_TWO_SIDED", "1u")):
        assert re.search(r"#define %s %s\b" % (define, value), HEADER) and getattr(_lib, define) == int(value.rstrip("u")), define
    section = HEADER.split("The floating bodies reflected in the water")[1].split("several devices")[0]
    for cite in ("water -> solids -> ow_shadow_apply -> ow_mirror_apply -> ow_environment_apply -> ow_mist_apply -> billboards -> ow_present", "ow_mirror.h",
                 "THIS LIBRARY'S CHOICE", "OW_RAY_MIRROR", "no group form", "the water reflected in itself", "shadows on the mirrored body",
                 "roughness blur of the mirrored image", "reflections in the\n *              spray", "bit for bit", "no water limit"):
        assert cite in section, cite
    note = open(os.path.join(CSRC, "ow_mirror.h")).read()
    for cite in ("THIS LIBRARY'S CHOICE", "-ffp-contract=off", "not here", "the water reflected in itself", "shadows on the mirrored body", "roughness blur",
                 "reflections in the spray", "a group form", "sky_light_begin", "solid_cast_pair", "glsl_mix"):
        assert cite in note, cite
    assert "ow_mirror.h's pass" in open(os.path.join(CSRC, "ow_sky_light.h")).read()
    o, so, lo = _lib.ow_mirror_options(), _lib.ow_solid_options(), _lib.ow_radiance_light_options()
    lib.ow_mirror_options_init(C.byref(o))
    lib.ow_solid_options_default(C.byref(so))
    lib.ow_radiance_light_options_default(C.byref(lo))
    assert (o.ambient_energy, o.reflection_energy, o.specular) == (lo.ambient_energy, lo.reflection_energy, lo.specular) == (1.0, 1.0, 0.5)
    assert list(o.body_color) == list(so.color) and list(o.light_direction) == list(so.light_direction)
    assert list(o.light_color) == list(so.light_color) and list(o.ambient_color) == list(so.ambient_color)
    assert (o.max_distance, o.fade_begin, o.opacity, o.flags, o.cull) == (200.0, 100.0, 1.0, 0, 0) and not any(o.reserved)
    lib.ow_mirror_options_init(None)


def test_structs_agree_in_c_ctypes_and_the_harness(tmp_path, harness):
    name, St = "ow_mirror_options", _lib.ow_mirror_options
    fields = [f for f, _ in St._fields_]
    expr = ", ".join(["sizeof(%s)" % name] + ["offsetof(%s, %s)" % (name, f) for f in fields])
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ocean_waves.h"\nint main(void){printf("%s\\n", ' % " ".join(["%zu"] * (1 + len(fields)))
           + expr + ");return 0;}\n")
    vals = layout_probe(tmp_path, name + "_layout", src)
    assert vals == [C.sizeof(St)] + [getattr(St, f).offset for f in fields] and vals[0] == 128
    assert vals[1:] == [0, 4, 8, 12, 24, 36, 48, 60, 64, 68, 72, 76, 80]
    sizes = (C.c_int * 16)()
    harness.harness_mirror_sizes(sizes)
    assert list(sizes) == [128] + vals[4:] + [CASE.itemsize, 26, MIRROR, _lib.OW_MIRROR_TWO_SIDED, 0]
    # the option bytes: what the wrapper fills is what the header lays out
    o = mirror.mirror_options(dict(ambient_energy=0.25, body_color=(1, 2, 3), light_direction=(4, 5, 6), light_color=(7, 8, 9), ambient_color=(10, 11, 12),
                                   max_distance=50.0, fade_begin=20.0, opacity=0.5, cull=-1, two_sided=True))
    words = np.frombuffer(bytes(o), np.float32)
    assert list(words[[0, 1, 2]]) == [0.25, 1.0, 0.5] and list(words[3:15]) == [float(k) for k in range(1, 13)] and list(words[15:18]) == [50.0, 20.0, 0.5]
    assert list(np.frombuffer(bytes(o), np.int32)[18:20]) == [1, -1] and not np.frombuffer(bytes(o), np.uint32)[20:].any()


def test_the_documents_name_the_new_calls():
    for name in NEW_FUNCTIONS:
        assert "`%s`" % name in S.DOC.split("## 7. Index")[1], name
    for name in NEW_FUNCTIONS[1:]:
        assert re.search(r"\[DllImport\(Lib\)\]\s*public static extern \w+ %s\(" % name, S.SHIM), name
    order = "water -> solids -> ow_shadow_apply -> ow_mirror_apply -> ow_environment_apply -> ow_mist_apply -> billboards -> ow_present"
    for doc, words in (("README.md", ("ow_mirror_apply", "profiles/mirror_1024x4.txt")),
                       ("DESIGN.md", ("k_mirror_apply", "ow_mirror.hip", "ow_mirror.h", order)),
                       ("INTEGRATION.md", ("ow_mirror_apply_async", "OW_RAY_MIRROR", "OwMirrorOptions", order)),
                       ("profiles/EXPERIMENTS.md", ("k_mirror_apply",))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)
    for path in ("scripts/mirror_cost.py", "examples/mirror_host.c", "profiles/mirror_margins.txt", "profiles/mirror_1024x4.txt"):
        assert os.path.exists(os.path.join(ROOT, path)), path


def test_example_builds_as_c99(tmp_path):
    build.build_library()
    build_example(tmp_path, "mirror_host")


# ---- 2. every refusal, without a device -------------------------------------------------------------------------------------------------------

def test_argument_errors_without_a_device():
    lib = _lib.load()
    cam = level_camera(24, 12)
    rec = np.zeros((12, 24), W.RENDER_PIXEL)
    hits = np.zeros((12, 24), SC.SOLID_HIT)
    tf = np.zeros((2, 12), np.float32)
    fake = C.c_void_p(16)   # never read: every case fails before a handle is looked at

    def apply(camera, opts, rec_p=rec.ctypes.data, count=2, tf_p=tf.ctypes.data):
        cp, op = (C.byref(camera) if camera is not None else None), (C.byref(opts) if opts is not None else None)
        out = []
        for fn in (lib.ow_mirror_apply, lib.ow_mirror_apply_async):
            assert fn(None, fake, fake, fake, 0, count, cp, op, rec_p, hits.ctypes.data) == _lib.OW_ERR_INVALID
            out.append(lib.ow_last_error().decode())
        assert lib.ow_mirror_apply_instances(None, fake, fake, tf_p, count, cp, op, rec_p, hits.ctypes.data) == _lib.OW_ERR_INVALID
        third = lib.ow_last_error().decode()
        assert out[0] == out[1]
        return out[0], third

    def both(camera, opts, word, **kw):
        a, b = apply(camera, opts, **kw)
        assert word in a and word in b, (word, a, b)

    mo = mirror.mirror_options
    both(cam, None, "null context")                                                             # everything else is in order
    both(cam, mo(dict(ambient_energy=1e12, reflection_energy=0.0, specular=1.0, max_distance=1e12, fade_begin=0.0, opacity=0.0, cull=-1, two_sided=True)),
         "null context")
    both(cam, None, "the records", rec_p=None)
    both(None, None, "null camera")
    for w, h in ((0, 12), (24, 0), (_lib.OW_RENDER_MAX_SIDE + 1, 12)):
        both(level_camera(w, h), None, "camera size")
    bad = level_camera(24, 12)
    bad.reserved[1] = 7
    both(bad, None, "ow_camera.reserved")
    nan, inf = float("nan"), float("inf")
    for key, values in (("ambient_energy", (nan, inf, -1.0, 2e12)), ("reflection_energy", (nan, -1e-3, 2e12)), ("specular", (nan, -0.1, 1.1)),
                        ("max_distance", (nan, inf, 0.0, -1.0, 2e12)), ("opacity", (nan, -0.1, 1.1))):
        for v in values:
            both(cam, mo({key: v}), key)
    for fb, md in ((nan, 10.0), (-1.0, 10.0), (10.0, 10.0), (11.0, 10.0)):
        both(cam, mo(dict(fade_begin=fb, max_distance=md)), "fade_begin")
    for key in ("body_color", "light_direction", "light_color", "ambient_color"):
        for v in ((nan, 0, 1), (0, inf, 1), (2e12, 0, 1)):
            both(cam, mo({key: v}), "a colour or the light direction")
    both(cam, mo(dict(light_direction=(0, 0, 0))), "zero length")
    o = mo({})
    o.flags = 2
    both(cam, o, "unknown mirror flags")
    for c in (1, -2):
        both(cam, mo(dict(cull=c)), "cull")
    o = mo({})
    o.reserved[11] = 1
    both(cam, o, "ow_mirror_options.reserved")
    # the order: the records before the camera before the options, and an option's own order as the header lists them
    both(None, mo(dict(opacity=2.0)), "the records", rec_p=None)
    both(None, mo(dict(opacity=2.0)), "null camera")
    both(cam, mo(dict(specular=2.0, opacity=2.0)), "specular")
    # the transforms of the _instances form are looked at behind the options and ahead of the context
    a, b = apply(cam, None, count=-1)
    assert "null context" in a and "instance_count" in b
    a, b = apply(cam, None, count=_lib.OW_SOLID_MAX_INSTANCES + 1)
    assert "instance_count" in b
    a, b = apply(cam, None, tf_p=None)
    assert "null context" in a and "null argument" in b
    a, b = apply(cam, mo(dict(opacity=2.0)), count=-1)
    assert "opacity" in b
    assert lib.ow_mirror_stats(None, None, None, None, None, None, None) == _lib.OW_ERR_INVALID and "null context" in lib.ow_last_error().decode()
    assert not rec.tobytes().strip(b"\0") and not hits.tobytes().strip(b"\0")
    with pytest.raises(ValueError):
        mo(dict(density=1.0))


# ---- 3. the CPU build's bit identities ----------------------------------------------------------------------------------------------------------

def test_cpu_no_bodies_is_the_sky_pass(harness, pyramid, sky_pyramid):
    """without instances, and with every instance out of every ray's reach, the records are the sky-light harness's to the bit and every hit
    record is the no-hit record"""
    for (w, h) in PICTURES:
        cam = view_camera(w, h)
        rec = sea_records(cam, w)
        want = sky_pyramid.apply(rec, cam)["rec"]
        far = crates_over(5)
        far[:, 10] += 500.0                                                    # 500 m up: beyond max_distance 200 of every ray
        for what, shape, tf in (("no instances", None, None), ("a shape, no instances", SHAPES[12], np.zeros((0, 12))), ("out of reach", SHAPES[12], far)):
            got = cpu_mirror(harness, pyramid, cam, rec, shape, tf)
            same_records(got["rec"], want, what)
            assert got["hits"].tobytes() == no_hit_records(rec.shape).tobytes(), what
            assert got["rays_hit"] == 0 and got["pixels"] == int(((want["status"] ^ rec["status"]) & LIT != 0).sum()) > 50, what
            assert (got["rays_cast"] > 0) == (tf is not None and len(tf) > 0), what
        assert not ((want["status"] & MIRROR) != 0).any()


def reference_hits(cast_harness, sky, cam, rec, shape, tf, opts):
    """ow_cast_bodies' CPU build over the sky-light harness's reflect and the records' position, placed where the records cast"""
    o = options_of(opts)
    st = sky.apply(rec, cam, light_options(o))
    status = rec["status"]
    n = rec["normal"]
    casting = ((status & HIT) != 0) & ((status & (ENV | LIT | SOLID | BELOW)) == 0) & np.isfinite(n).all(-1) & (n != 0).any(-1) & (len(tf) > 0)
    want = no_hit_records(rec.shape)
    if casting.any():
        rays = W.rays(rec["position"][casting], st["reflect"][casting], o.max_distance)
        want[casting] = cpu_cast(cast_harness, shape, tf, rays, bool(o.flags & 1), o.cull)
    return want, casting


CAST_CASE = np.dtype([(k, np.int32) for k in ("num_vertices", "num_triangles", "count", "stride", "has_flags", "num_rays", "has_water", "two_sided", "cull")])


def cpu_cast(L, shape, tf, rays, two_sided, cull):
    """the records of the ray cast's CPU build (tests/solid_cast/solid_cast_harness.cpp) over [count][12] transforms, no water limit"""
    v = np.ascontiguousarray(shape[0], np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(shape[1], np.int32).reshape(-1, 3)
    tf = np.ascontiguousarray(tf, np.float32).reshape(-1)
    r = np.ascontiguousarray(rays, W.RAY).reshape(-1)
    h = np.zeros(1, CAST_CASE)
    h["num_vertices"], h["num_triangles"], h["count"], h["stride"], h["num_rays"], h["two_sided"], h["cull"] = len(v), len(t), tf.size // 12, 12, len(r), int(two_sided), cull
    out = np.zeros(len(r), SC.SOLID_HIT)
    counters = np.zeros(3, np.uint64)
    L.harness_solid_cast(h.ctypes.data, v.ctypes.data, t.ctypes.data, tf.ctypes.data, None, r.ctypes.data, None, out.ctypes.data, counters.ctypes.data, None, None)
    return out


@pytest.fixture(scope="module")
def cast_harness():
    L = harness_library("solid_cast")
    L.harness_solid_cast.argtypes = [C.c_void_p] * 11
    return L


def test_cpu_the_hit_is_the_casts(harness, pyramid, sky_pyramid, cast_harness):
    """for every casting record the hit record is the ray cast's CPU build's on (position, reflect), one- and two-sided; for every other
    record the no-hit record; a position that is not finite gives the cast's invalid record"""
    cam = view_camera(*PICTURES[0])
    rec = sea_records(cam, 3, far=True)
    for nt in (1, 12, 65):
        for count in (1, 65):
            tf = crates_over(count)
            for two_sided in (False, True):
                opts = dict(two_sided=two_sided)
                got = cpu_mirror(harness, pyramid, cam, rec, SHAPES[nt], tf, opts)
                want, casting = reference_hits(cast_harness, sky_pyramid, cam, rec, SHAPES[nt], tf, opts)
                assert got["hits"].tobytes() == want.tobytes(), (nt, count, two_sided)
                assert np.array_equal(got["cast"], casting) and got["rays_cast"] == int(casting.sum())
                assert got["rays_hit"] == int(((want["status"] & HIT) != 0).sum())
    assert (want["status"] == INVALID).sum() == 2 and ((want["status"] & HIT) != 0).sum() > 5


def test_cpu_culling_twice_and_after_the_sky_pass(harness, pyramid, sky_pyramid):
    cam = view_camera(*PICTURES[1])
    rec = sea_records(cam, 5)
    shape, tf = SHAPES[12], crates_over(64)
    a = cpu_mirror(harness, pyramid, cam, rec, shape, tf)
    b = cpu_mirror(harness, pyramid, cam, rec, shape, tf, dict(cull=-1))
    same_records(a["rec"], b["rec"], "cull")
    assert a["hits"].tobytes() == b["hits"].tobytes() and a["rays_hit"] == b["rays_hit"] > 5 and a["skipped"] == b["skipped"] == 1
    assert a["cull_mistakes"] == 0 and a["cull_dropped"] > 0
    assert b["sphere_tests_passed"] == 63 * b["rays_cast"] > a["sphere_tests_passed"] > 0 and b["pairs_tested"] == 12 * b["sphere_tests_passed"]
    mirrored = (a["rec"]["status"] & MIRROR) != 0
    assert mirrored.sum() > 5 and not (mirrored & ~a["cast"]).any()
    for f in W.RENDER_PIXEL.names:                                              # only color and status change
        if f not in ("color", "status"):
            assert a["rec"][f].tobytes() == rec[f].tobytes(), f
    twice = cpu_mirror(harness, pyramid, cam, a["rec"], shape, tf)
    same_records(twice["rec"], a["rec"], "twice")
    assert twice["pixels"] == twice["rays_cast"] == 0 and twice["hits"].tobytes() == no_hit_records(rec.shape).tobytes()
    lit = sky_pyramid.apply(rec, cam)["rec"]
    same_records(cpu_mirror(harness, pyramid, cam, lit, shape, tf)["rec"], lit, "after the sky pass")
    # where no body is met the record is the sky pass's, where one is it is not
    assert np.array_equal((a["rec"]["color"] != lit["color"]).any(-1), mirrored)
    assert np.array_equal(a["rec"]["status"] & ~MIRROR, lit["status"])
    bad = level_camera(24, 16)
    bad.position[0] = np.nan
    dead = cpu_mirror(harness, pyramid, bad, rec, shape, tf)                   # a camera that is not finite changes nothing
    same_records(dead["rec"], rec, "camera")
    assert dead["hits"].tobytes() == no_hit_records(rec.shape).tobytes()


def test_cpu_the_tile_cull_drops_nothing_a_lane_passes(harness, pyramid):
    """The kernel drops, for a whole tile, the instances mirror_bundle_pass refuses.  The CPU build, which walks every instance on every
    lane, counts the (tile, instance) pairs the test refuses although a lane of the tile passes the sphere test: none, on seas seen from
    0.2 m to 400 m up, level and steep, with instances from 0.01 to 300 m in size near, far, behind the camera and beyond max_distance,
    and max_distance from 1 m to 1e12; and the cull does work: most pairs are dropped"""
    rng = np.random.default_rng(77)
    tested = dropped = 0
    for k in range(24):
        w, h = PICTURES[k % 2]
        height = float(rng.choice([0.2, 1.0, 3.0, 12.0, 80.0, 400.0]))
        cam = look(position=(rng.uniform(-50, 50), height, rng.uniform(-50, 50)), yaw_deg=rng.uniform(-180, 180), pitch_deg=-float(rng.choice([1.0, 8.0, 30.0, 75.0])),
                   fov=float(rng.choice([20.0, 75.0, 120.0])), width=w, height=h, max_distance=1e5)
        rec = sea_records(cam, 100 + k, ripple=float(rng.choice([0.0, 0.03, 0.5])))
        n = int(rng.choice([5, 70, 200]))
        span = float(rng.choice([10.0, 100.0, 3000.0]))
        rows = []
        for _ in range(n):
            q = rng.normal(size=4)
            rows.append(((cam.position[0] + rng.uniform(-span, span), rng.uniform(-2.0, 0.3 * span), cam.position[2] + rng.uniform(-span, span)), q / np.linalg.norm(q),
                         float(rng.choice([0.01, 1.0, 5.0, 150.0]))))
        md = float(rng.choice([1.0, 30.0, 200.0, 1e4, 1e12]))
        got = cpu_mirror(harness, pyramid, cam, rec, SHAPES[12], transforms(rows), dict(max_distance=md, fade_begin=0.5 * md, two_sided=bool(k % 2)))
        assert got["cull_mistakes"] == 0, (k, got["cull_tested"], got["cull_dropped"])
        tested += got["cull_tested"]
        dropped += got["cull_dropped"]
    print("tile cull:", tested, "pairs tested,", dropped, "dropped")
    assert tested > 10000 and dropped > 0.5 * tested


# ---- 4. the FP64 twin ---------------------------------------------------------------------------------------------------------------------------

TWIN_CAM = dict(position=(0.3, 3.0, -2.0), yaw_deg=3.0, pitch_deg=-14.0, fov=75.0, width=96, height=64, max_distance=4000.0)


def twin_crates():
    """24 boxes of (2, 1, 2) m scaled 1 to 2, tumbled, 6 to 30 m in front of the camera: each several pixels across at 96 x 64; no slivers"""
    rng = np.random.default_rng(2026)
    rows = []
    for k in range(24):
        q = rng.normal(size=4)
        rows.append((((k % 6 - 2.5) * 3.0 + rng.uniform(-0.5, 0.5), rng.uniform(0.6, 2.4), 6.0 + 6.0 * (k // 6) + rng.uniform(-1, 1)), q / np.linalg.norm(q),
                     rng.uniform(1.0, 2.0)))
    return transforms(rows)


def measure_twin(harness, pyramid, two_sided):
    cam = look(**TWIN_CAM)
    rec = sea_records(cam, 9)
    shape, tf = SHAPES[12], twin_crates()
    opts = dict(two_sided=two_sided, max_distance=60.0, fade_begin=10.0, opacity=0.9)
    got = cpu_mirror(harness, pyramid, cam, rec, shape, tf, opts)
    o = options_of(opts)
    pyr = SL.pyramid(PANO["image"], PANO["srgb"], PANO["energy"], ROPTS["levels"], ROPTS["samples"], RADIANCE_DEFAULTS["base_width"])
    tw = MT.mirror(rec, camera_words(cam), values_of(o), pyr, shape, tf)
    assert np.array_equal(got["cast"], tw["cast"]) and got["cull_mistakes"] == 0
    build_pair = np.where((got["hits"]["status"] & HIT) != 0, got["hits"]["instance"] * 12 + got["hits"]["triangle"], -1)
    same = build_pair == tw["pair"]
    casting = int(tw["cast"].sum())
    differ = np.argwhere(~same & tw["cast"])
    # a ray that grazes an edge may pick the neighbouring pair in FP32: for each such pixel the twin's t for the build's pair is the build's
    # t within the cast test's own tolerance (one FP32 ulp), or the build missed what the twin grazed
    order = np.cumsum(tw["cast"].ravel()).reshape(tw["cast"].shape) - 1
    for j, i in differ:
        if build_pair[j, i] >= 0:
            t = f32(MT.pair_t(shape, tf, tw["rays"][order[j, i]], int(build_pair[j, i])))
            ulp = abs(int(t.view(np.int32)) - int(got["hits"]["t"][j, i].view(np.int32)))
            assert ulp <= 1, (j, i, ulp)
        assert not tw["unambiguous"][j, i], (j, i)
    share = len(differ) / max(casting, 1)
    keep = same | ~tw["cast"]
    err = rel(got["rec"]["color"][keep], tw["color"][keep])
    assert np.array_equal(got["rec"]["status"][keep], tw["status"][keep])
    hits = int(tw["hit"].sum())
    print(f"two_sided {two_sided}: casting {casting} hits {hits} pairs that differ {len(differ)} share {share:.5f} largest colour error {err:.3e}")
    return dict(casting=casting, hits=hits, share=share, color=err)


def test_cpu_build_against_the_fp64_twin(harness, pyramid):
    """The colour within test_sky_light's tolerance for color (1e-4 relative to max(1, |value|)) wherever the twin's winning pair is the
    build's; the other casting pixels are at most 0.5 % of the casting pixels.  Observed (profiles/mirror_margins.txt): no pair differs and
    the largest colour error is a few 1e-7."""
    for two_sided in (False, True):
        m = measure_twin(harness, pyramid, two_sided)
        assert m["casting"] > 2000 and m["hits"] > 150, m
        assert m["share"] <= 0.005, m
        assert m["color"] <= TOL_F32, m


# ---- 5. the closed form -----------------------------------------------------------------------------------------------------------------------

CLOSED = dict(h=2.0, d=16.0, half_x=4.0, top=4.0)


def closed_form_case():
    """A flat sea (normal (0, 1, 0), positions on y = 0) seen from (0, h, 0), and one box whose vertical face at z = d spans |x| <= 4 and
    0 <= y <= 4.  The mirror ray from (x0, 0, z0) has direction (x0, h, z0) / L, L = |(x0, h, z0)|, and meets the plane z = d at
    t = L (d - z0) / z0, at x = x0 d / z0 and at height h (d - z0) / z0."""
    h, d = CLOSED["h"], CLOSED["d"]
    pts = [(0.0, 8.0), (0.0, 12.0), (1.0, 8.0), (-1.25, 6.0), (0.0, 4.0), (0.0, 5.0), (3.0, 8.0), (0.5, 15.0), (0.0, 2.0), (-2.0, 15.5), (1.0, 10.0), (0.25, 7.0)]
    cam = level_camera(4, 3, position=(0.0, h, 0.0))
    rec = np.zeros((3, 4), W.RENDER_PIXEL)
    rec["status"] = HIT
    rec["position"] = np.float32([(x, 0.0, z) for x, z in pts]).reshape(3, 4, 3)
    rec["normal"] = (0.0, 1.0, 0.0)
    rec["albedo"], rec["roughness"], rec["color"] = (0.02, 0.03, 0.04), 0.1, (0.01, 0.02, 0.03)
    rec["t"] = np.linalg.norm(rec["position"] - f32([0.0, h, 0.0]), axis=-1)
    shape = box((8.0, 4.0, 2.0))
    tf = transforms([((0.0, 2.0, d + 1.0),)])
    x0, z0 = np.float64([p[0] for p in pts]).reshape(3, 4), np.float64([p[1] for p in pts]).reshape(3, 4)
    L = np.sqrt(x0 * x0 + h * h + z0 * z0)
    want = dict(t=L * (d - z0) / z0, x=x0 * d / z0, y=h * (d - z0) / z0)
    want["hit"] = (np.abs(want["x"]) < CLOSED["half_x"]) & (want["y"] < CLOSED["top"])
    return cam, rec, shape, tf, want


def check_closed_form(apply, sky_apply):
    """apply(cam, rec, shape, tf, opts) -> (records, hits); sky_apply(cam, rec) -> the sky pass's records.

    The bound.  V = -(position - camera) / len: the subtraction is exact for these dyadic values, len = sqrtf(dot3) carries at most 1.5 ulp,
    the division half an ulp more, so each component of V is within 2 ulp.  With N = (0, 1, 0): nv = V.y and R = (-V.x, 2 V.y - V.y, -V.z) exactly.
    ray_setup divides by |R| = 1 within 2.5 ulp (a dot product and a square root) and rounds: d^ within 5 ulp per component.  The pair's FP64 arithmetic
    on the exact dyadic vertices adds nothing, its narrowing half an ulp: t = (d - z0) / d^.z within 5.5 ulp, allowed 8 ulp = 8 x 2^-23 t.
    position_k = o_k + t d^_k in FP32: t d^_k within (5.5 + 5 + 0.5) ulp of itself, the sum half an ulp of the larger of its terms and the
    result: allowed 16 x 2^-23 max(|o_k|, |t d^_k|, |position_k|) <= 16 x 2^-23 max(d, t)."""
    cam, rec, shape, tf, want = closed_form_case()
    out, hits = apply(cam, rec, shape, tf, None)
    sky = sky_apply(cam, rec)
    hit = (hits["status"] & HIT) != 0
    assert np.array_equal(hit, want["hit"]) and 4 <= hit.sum() <= 10 and (~hit).sum() >= 2
    ulp = 2.0 ** -23
    t = hits["t"].astype(np.float64)
    assert (np.abs(t - want["t"])[hit] <= 8 * ulp * want["t"][hit]).all(), np.abs(t - want["t"])[hit] / (ulp * want["t"][hit])
    scale = np.maximum(CLOSED["d"], want["t"])
    for k, w in ((0, want["x"]), (1, want["y"]), (2, np.full(hit.shape, CLOSED["d"]))):
        e = np.abs(hits["position"][..., k].astype(np.float64) - w)
        assert (e[hit] <= 16 * ulp * scale[hit]).all(), (k, e[hit] / (ulp * scale[hit]))
    assert (hits["normal"][hit] == f32([0.0, 0.0, -1.0])).all() and (hits["instance"][hit] == 0).all() and np.isin(hits["triangle"][hit], (8, 9)).all()
    assert np.array_equal((out["status"] & MIRROR) != 0, hit)
    over = ~hit                                                                 # the ray passes over (or beside) the box: the sky pass's colour
    assert out["color"][over].tobytes() == sky["color"][over].tobytes() and (out["status"][over] == sky["status"][over]).all()
    assert (out["color"][hit] != sky["color"][hit]).any(-1).all()
    assert hits[over].tobytes() == no_hit_records(hit.shape)[over].tobytes()


def test_cpu_closed_form(harness, pyramid, sky_pyramid):
    def apply(cam, rec, shape, tf, opts):
        g = cpu_mirror(harness, pyramid, cam, rec, shape, tf, opts)
        return g["rec"], g["hits"]
    check_closed_form(apply, lambda cam, rec: sky_pyramid.apply(rec, cam)["rec"])


# ---- 6. fade and opacity ------------------------------------------------------------------------------------------------------------------------

def check_fade_and_opacity(apply, sky_apply, harness, pyramid):
    """opacity 0: the sky pass's colours with OW_RAY_MIRROR on the same pixels as at opacity 1.  At t <= fade_begin and opacity 1 radiance' is
    C to the bit: the colour is color + (ambient + (C scale) reflection_energy) in FP32, C, ambient and env being the CPU build's stages."""
    cam = view_camera(*PICTURES[1])
    rec = sea_records(cam, 7, kinds=False)
    shape, tf = SHAPES[12], crates_over(12, seed=4, z=(2.0, 14.0))
    full, hits = apply(cam, rec, shape, tf, dict(opacity=1.0, fade_begin=30.0, max_distance=60.0))
    none, _ = apply(cam, rec, shape, tf, dict(opacity=0.0, fade_begin=30.0, max_distance=60.0))
    sky = sky_apply(cam, rec)
    mirrored = (full["status"] & MIRROR) != 0
    assert mirrored.sum() > 10 and np.array_equal((none["status"] & MIRROR) != 0, mirrored)
    assert none["color"].tobytes() == sky["color"].tobytes() and np.array_equal(none["status"] & ~MIRROR, sky["status"])
    st = cpu_mirror(harness, pyramid, cam, rec, shape, tf, dict(opacity=1.0, fade_begin=30.0, max_distance=60.0))
    near = mirrored & (hits["t"] <= 30.0)
    assert near.sum() > 10 and (st["weight"][near] == 1.0).all()
    assert st["radiance"][near].tobytes() == st["body"][near].tobytes()
    f0 = f32(0.16) * f32(0.5) * f32(0.5)
    f50 = min(max(f32(50.0) * f0, f32(0.0)), f32(1.0))
    scale = st["env"][..., 0] * f0 + st["env"][..., 1] * f50
    want = rec["color"] + (st["ambient"] + (st["body"] * scale[..., None]) * f32(1.0))
    assert want.dtype == np.float32 and full["color"][near].tobytes() == want[near].tobytes()
    beyond = mirrored & (hits["t"] > 30.0)                                      # the fade: weights strictly between 0 and 1
    if beyond.any():
        assert ((st["weight"][beyond] > 0) & (st["weight"][beyond] < 1)).all()
    faded, _ = apply(cam, rec, shape, tf, dict(opacity=1.0, fade_begin=1.0, max_distance=np.nextafter(f32(hits["t"][near].max()), f32(1e9))))
    assert ((faded["status"] & MIRROR) != 0).sum() > 0


def test_cpu_fade_and_opacity(harness, pyramid, sky_pyramid):
    def apply(cam, rec, shape, tf, opts):
        g = cpu_mirror(harness, pyramid, cam, rec, shape, tf, opts)
        return g["rec"], g["hits"]
    check_fade_and_opacity(apply, lambda cam, rec: sky_pyramid.apply(rec, cam)["rec"], harness, pyramid)


# ---- 7. the device ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def device():
    gen = bare_context()
    sky, radiance = gpu_radiance(gen, PANO, ROPTS)
    solids = {nt: gen.solid_create(*SHAPES[nt]) for nt in SHAPES}
    yield dict(gen=gen, radiance=radiance, solids=solids)
    for s in solids.values():
        gen.solid_destroy(s)
    gen.radiance_destroy(radiance)
    gen.sky_destroy(sky)
    gen.free()


def gpu_instances(device, cam, rec, nt, tf, opts=None):
    """the host form over a caller's transforms: (records, hits, the counters)"""
    gen = device["gen"]
    out, hits = mirror.mirror_apply_instances(gen, device["radiance"], cam, rec, device["solids"][nt] if nt else None, tf, opts, hits=True)
    return out, hits, mirror.mirror_stats(gen)


def same_as_cpu(got, stats, want, what):
    out, hits = got
    same_records(out, want["rec"], what)
    assert hits.tobytes() == want["hits"].tobytes(), what
    assert {k: stats[k] for k in COUNTERS} == {k: want[k] for k in COUNTERS}, what


@pytest.mark.gpu
def test_gpu_no_bodies_is_the_sky_pass(device):
    """1. body_count 0, a NULL solid, and instances out of every ray's reach: the records are ow_radiance_light_apply's, the hits no-hit"""
    gen, radiance = device["gen"], device["radiance"]
    for (w, h) in PICTURES:
        cam = view_camera(w, h)
        rec = sea_records(cam, w)
        want = gen.sky_light_apply(radiance, cam, rec)
        empty = no_hit_records(rec.shape).tobytes()
        out, hits = mirror.mirror_apply(gen, radiance, cam, rec, hits=True)                                     # a NULL solid
        same_records(out, want, "NULL solid")
        assert hits.tobytes() == empty
        out, hits, _ = gpu_instances(device, cam, rec, 12, np.zeros((0, 12), np.float32))                       # a solid, no instances
        same_records(out, want, "no instances")
        assert hits.tobytes() == empty
        far = crates_over(5)
        far[:, 10] += 500.0
        for opts in (None, dict(cull=-1)):
            out, hits, stats = gpu_instances(device, cam, rec, 12, far, opts)
            same_records(out, want, ("out of reach", opts))
            assert hits.tobytes() == empty and stats["rays_hit"] == 0 and stats["rays_cast"] > 50
        same_records(mirror.mirror_apply(gen, radiance, cam, rec), want, "no hits asked for")


@pytest.mark.gpu
def test_gpu_the_hit_is_the_casts(device, sky_pyramid):
    """2. for every casting record hits_out is ow_cast_instances' record for (position, the sky-light harness's reflect), one- and two-sided;
    for every other record the no-hit record"""
    gen = device["gen"]
    cam = view_camera(*PICTURES[0])
    rec = sea_records(cam, 3, far=True)
    st = sky_pyramid.apply(rec, cam)
    n, status = rec["normal"], rec["status"]
    casting = ((status & HIT) != 0) & ((status & (ENV | LIT | SOLID | BELOW)) == 0) & np.isfinite(n).all(-1) & (n != 0).any(-1)
    rays = W.rays(rec["position"][casting], st["reflect"][casting], 200.0)
    for nt, count in ((1, 65), (12, 64), (65, 63)):
        tf = crates_over(count)
        for two_sided in (False, True):
            want = no_hit_records(rec.shape)
            want[casting] = SC.raycast_solids_instances(gen, device["solids"][nt], tf, rays, options=dict(two_sided=two_sided))
            _, hits, stats = gpu_instances(device, cam, rec, nt, tf, dict(two_sided=two_sided))
            assert hits.tobytes() == want.tobytes(), (nt, count, two_sided)
            assert stats["rays_cast"] == int(casting.sum()) and stats["rays_hit"] == int(((want["status"] & HIT) != 0).sum())
    assert ((want["status"] & HIT) != 0).sum() > 5 and (want["status"] == INVALID).sum() == 2


@pytest.mark.gpu
def test_gpu_equals_the_cpu_build_on_hand_built_records(device, harness, pyramid):
    """3. records of every kind, both picture sizes, the chunk edges of the instance count, shapes of 1, 12 and 65 triangles, one instance
    with a transform that is not finite, with and without culling: records, hits and counters bit for bit"""
    total = 0
    for k, count in enumerate(COUNTS):
        for m, nt in enumerate((1, 12, 65)):
            w, h = PICTURES[(k + m) % 2]
            cam = view_camera(w, h)
            rec = sea_records(cam, 20 + k)
            tf = crates_over(count)
            opts = dict(two_sided=bool((k + m) % 3 == 0), max_distance=80.0, fade_begin=8.0, opacity=0.8)
            want = cpu_mirror(harness, pyramid, cam, rec, SHAPES[nt], tf, opts)
            for cull in (0, -1):
                want = want if cull == 0 else cpu_mirror(harness, pyramid, cam, rec, SHAPES[nt], tf, dict(opts, cull=cull))
                out, hits, stats = gpu_instances(device, cam, rec, nt, tf, dict(opts, cull=cull))
                same_as_cpu((out, hits), stats, want, (count, nt, cull))
            total += want["rays_hit"]
    assert total > 100


@pytest.mark.gpu
def test_gpu_equals_the_cpu_build_on_a_drawn_scene(harness, pyramid):
    """3. tests/scenes.py' sea with crates at 1024^2 x 3, drawn small from low over the water: the set's resident poses on the device against
    the CPU build on the same pose records"""
    gen, params, sc, bodies, spray = frame_scene(n=1024)
    cam = look(position=(-1.0, 2.5, -62.0), yaw_deg=0.0, pitch_deg=-5.0, fov=60.0, width=72, height=40, max_distance=4000.0)
    mesh = gen.mesh_create(*grid(*FRAME_WATER))
    dark = (0.0, 0.0, 0.0)
    _, bg = gen.mesh_draw(mesh, cam, W.clipmap_origin(cam.position, FRAME_WATER[1]), sc, {"falloff": True, "cull_back": True, "ambient_color": dark})
    solid = gen.solid_create(*box(FRAME_SHAPE))
    _, mid = gen.solid_draw(solid, bodies, cam, {"ambient_color": dark}, pixels=bg)
    sky, radiance = gpu_radiance(gen, PANO, ROPTS)
    poses = pose_transforms(gen, bodies)
    for cull in (0, -1):
        out, hits = mirror.mirror_apply(gen, radiance, cam, mid, solid, bodies, dict(cull=cull), hits=True)
        stats = mirror.mirror_stats(gen)
        want = cpu_mirror(harness, pyramid, cam, mid, box(FRAME_SHAPE), poses, dict(cull=cull), stride=24)
        same_as_cpu((out, hits), stats, want, cull)
        assert want["cull_mistakes"] == 0
    water = ((mid["status"] & HIT) != 0) & ((mid["status"] & SOLID) == 0)
    print("water", int(water.sum()), "solid", int(((mid["status"] & SOLID) != 0).sum()), stats)
    assert water.sum() > 500 and stats["rays_cast"] > 500 and stats["rays_hit"] > 0
    assert not ((out["status"] & MIRROR) != 0)[~water].any()
    for h_, fn in ((radiance, gen.radiance_destroy), (sky, gen.sky_destroy), (solid, gen.solid_destroy), (mesh, gen.mesh_destroy), (bodies, gen.bodies_destroy),
                   (spray, gen.spray_destroy)):
        fn(h_)
    gen.free()


@pytest.mark.gpu
def test_gpu_the_organisation_does_not_show(device):
    """4. cull 0 and -1, the _async, host and _instances forms, a body set and its poses as transforms: the same bytes; a
    second application and an application after ow_radiance_light_apply change nothing; the async form does not synchronise"""
    import torch
    gen, radiance, solid = device["gen"], device["radiance"], device["solids"][12]
    cam = view_camera(*PICTURES[0])
    rec = sea_records(cam, 31)
    rng = np.random.default_rng(8)
    items = []
    for k in range(20):
        q = rng.normal(size=4)
        items.append(crate(origin=(rng.uniform(-8, 8), rng.uniform(0.4, 2.5), rng.uniform(2, 30)), q=tuple(q / np.linalg.norm(q)), density=0.0))
    bodies = gen.bodies_create(*make_bodies(items))
    poses = pose_transforms(gen, bodies)[:, :12]
    base, base_hits = mirror.mirror_apply(gen, radiance, cam, rec, solid, bodies, hits=True)
    stats = mirror.mirror_stats(gen)
    assert stats["rays_hit"] > 5 and ((base["status"] & MIRROR) != 0).sum() > 5
    for opts in (dict(cull=-1), dict(cull=-1, two_sided=False)):
        out, hits = mirror.mirror_apply(gen, radiance, cam, rec, solid, bodies, opts, hits=True)
        same_records(out, base, opts)
        assert hits.tobytes() == base_hits.tobytes(), opts
    out, hits = mirror.mirror_apply_instances(gen, radiance, cam, rec, solid, poses, hits=True)                 # the poses as transforms
    same_records(out, base, "instances")
    assert hits.tobytes() == base_hits.tobytes()
    part, part_hits = mirror.mirror_apply(gen, radiance, cam, rec, solid, bodies, first=3, count=9, hits=True)  # a range of the set
    out, hits = mirror.mirror_apply_instances(gen, radiance, cam, rec, solid, poses[3:12], hits=True)
    same_records(part, out, "range")
    assert part_hits.tobytes() == hits.tobytes() and part_hits.tobytes() != base_hits.tobytes()
    _, rec_dev = device_buffers(cam)
    hits_dev = torch.zeros((cam.width * cam.height, SC.SOLID_HIT.itemsize), dtype=torch.uint8, device="cuda:0")
    rec_dev.copy_(torch.from_numpy(np.frombuffer(rec.tobytes(), np.uint8).reshape(-1, 128).copy()))
    mirror.mirror_apply_async(gen, radiance, cam, rec_dev, solid, bodies)                                        # warm: the scratch is there
    torch.cuda.synchronize()                                                                                     # the copy below is on another stream
    rec_dev.copy_(torch.from_numpy(np.frombuffer(rec.tobytes(), np.uint8).reshape(-1, 128).copy()))
    torch.cuda.synchronize()
    syncs = gen.sync_stats()
    mirror.mirror_apply_async(gen, radiance, cam, rec_dev, solid, bodies, hits_dev)
    assert gen.sync_stats() == syncs
    torch.cuda.synchronize()
    same_records(records_of(cam, rec_dev), base, "async")
    assert hits_dev.cpu().numpy().tobytes() == base_hits.tobytes()
    mirror.mirror_apply_async(gen, radiance, cam, rec_dev, solid, bodies, hits_dev)                              # twice is once
    torch.cuda.synchronize()
    same_records(records_of(cam, rec_dev), base, "twice")
    assert hits_dev.cpu().numpy().tobytes() == no_hit_records(rec.shape).tobytes()
    lit = gen.sky_light_apply(radiance, cam, rec)
    same_records(mirror.mirror_apply(gen, radiance, cam, lit, solid, bodies), lit, "after the sky pass")
    # refusals on a live context: the shape, the set and the ranges, as ow_cast_bodies refuses them; nothing is written
    for call in (lambda: mirror.mirror_apply(gen, radiance, cam, rec, None, bodies),                            # bodies without a solid
                 lambda: mirror.mirror_apply(gen, radiance, cam, rec, solid, bodies, first=15, count=6),
                 lambda: mirror.mirror_apply_async(gen, radiance, cam, rec_dev.data_ptr() + 4, solid, bodies),
                 lambda: mirror.mirror_apply_async(gen, radiance, cam, rec_dev, solid, bodies, hits_dev.data_ptr() + 2)):
        with pytest.raises(_lib.OceanWavesError):
            call()
    torch.cuda.synchronize()
    same_records(records_of(cam, rec_dev), base, "after the refusals")
    gen.bodies_destroy(bodies)


@pytest.mark.gpu
def test_gpu_closed_form(device):
    """5. one box over a flat sea: the hit's position and t against the closed form within the bound check_closed_form derives"""
    gen, radiance = device["gen"], device["radiance"]
    solid = gen.solid_create(*box((8.0, 4.0, 2.0)))
    check_closed_form(lambda cam, rec, shape, tf, opts: mirror.mirror_apply_instances(gen, radiance, cam, rec, solid, tf, opts, hits=True),
                      lambda cam, rec: gen.sky_light_apply(radiance, cam, rec))
    gen.solid_destroy(solid)


@pytest.mark.gpu
def test_gpu_fade_and_opacity(device, harness, pyramid):
    """6. opacity 0 gives the sky pass's colours with OW_RAY_MIRROR where opacity 1 sets it; at t <= fade_begin and opacity 1 radiance' is C"""
    gen, radiance = device["gen"], device["radiance"]
    check_fade_and_opacity(lambda cam, rec, shape, tf, opts: mirror.mirror_apply_instances(gen, radiance, cam, rec, device["solids"][12], tf, opts, hits=True),
                           lambda cam, rec: gen.sky_light_apply(radiance, cam, rec), harness, pyramid)


@pytest.mark.gpu
def test_gpu_the_example_runs(tmp_path):
    """7. examples/mirror_host.c at 256^2 writes a 96 x 64 PPM of the frame through ow_mirror_apply, the same frame through
    ow_radiance_light_apply and each pixel's kind: the two differ in at least one water pixel and in no solid or sky pixel"""
    exe = build_example(tmp_path, "mirror_host")
    ppm, ref, kinds = str(tmp_path / "mirror.ppm"), str(tmp_path / "sky.ppm"), str(tmp_path / "kinds.bin")
    r = subprocess.run([exe, ppm, "96", "64", "40", "256", ref, kinds], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    kv = dict(p.split("=") for p in r.stdout.split())
    head = b"P6\n96 64\n255\n"
    a, b = open(ppm, "rb").read(), open(ref, "rb").read()
    assert a.startswith(head) and b.startswith(head) and len(a) == len(b) == len(head) + 96 * 64 * 3
    kind = np.frombuffer(open(kinds, "rb").read(), np.uint8).reshape(64, 96)
    differ = (np.frombuffer(a[len(head):], np.uint8).reshape(64, 96, 3) != np.frombuffer(b[len(head):], np.uint8).reshape(64, 96, 3)).any(-1)
    print(r.stdout, int(differ.sum()))
    assert (kind == 0).sum() > 100 and (kind == 1).sum() > 1000 and (kind == 2).sum() > 50
    assert differ[kind == 1].sum() >= 1 and not differ[kind != 1].any()
    assert int(kv["differing_water_pixels"]) == int(differ.sum()) and int(kv["differing_other_pixels"]) == 0
    assert kv["finite"] == "1" and int(kv["mirror_pixels"]) >= int(kv["differing_water_pixels"]) and int(kv["rays_hit"]) == int(kv["mirror_pixels"])
    assert int(kv["water_pixels"]) == int((kind == 1).sum()) and int(kv["crate_pixels"]) == int((kind == 2).sum())

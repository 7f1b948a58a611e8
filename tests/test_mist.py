"""Height mist with sun shafts over camera pictures (include/ocean_waves.h ow_mist_*, godotoceanwaves_amd/csrc/ow_mist.h).

CPU: the ABI, the documents and the argument checks without a device; ow_mist.h compiled as plain C++ (tests/mist/mist_harness.cpp, g++
-ffp-contract=off) held to an FP64 twin written from the header's text (tests/mist_twin.py) on the closed form's awkward rays (near-horizontal
ones within the same margin as the steep ones: profiles/mist_margins.txt holds the differences measured, the tests allow four times each),
to its bit identities (no map, a map never begun, an empty map and a map nobody looks behind are the same bytes; twice is once; slices 0
is 64; skipping the slices outside the frame's box changes no bit), to the twin's shafts behind one crate, and to finite outputs on fuzzed
options; the stand-alone harness runs under the sanitizers; the C example compiles.  GPU: k_mist_apply is the CPU build's bit for bit with
and without RGBA8; the asynchronous form in stream order equals the host form; the counters; a whole frame through ow_present;
examples/mist_host.c writes the wrapper's picture."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mist_twin as MT
import shadow_twin as ST
from godotoceanwaves_amd import _lib, build, mist
from godotoceanwaves_amd.presets import UPDATE_DELTA
from godotoceanwaves_amd.wave_generator import WaveGenerator as W
import checks as S
from checks import check_declared_and_bound, exported_symbols, HEADER
from cpu_builds import build_example, build_sanitized_harness, CSRC, harness_library, layout_probe, ROOT
from cpu_builds import shadow_harness  # noqa: F401 (fixture)
from scenes import (box, camera_words, CRATE_SHAPE, cube, device_buffers, eight_crates, example_crates, grid, HIT, level_camera, look, make_gen, records_of,
                    REF_BASIS, scales_of, SUN, synthetic_records, transforms)

MARGINS = os.path.join(ROOT, "profiles", "mist_margins.txt")
NEW_FUNCTIONS = ("ow_mist_options_init", "ow_mist_apply", "ow_mist_apply_async", "ow_mist_stats")
MIST, SOLID = _lib.OW_RAY_MIST, _lib.OW_RAY_SOLID
FLT_MAX_BITS = 0x7F7FFFFF
CASE = np.dtype([("width", np.int32), ("height", np.int32), ("size", np.int32), ("has_map", np.int32), ("cam", np.float32, 15), ("pad", np.int32),
                 ("options", np.uint8, 128), ("frame", np.uint8, 64)])


# ---- the CPU build ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def harness():
    L = harness_library("mist")
    V, I, F = C.c_void_p, C.c_int, C.c_float
    L.harness_mist_sizes.argtypes = [V]
    L.harness_mist_phi.argtypes = [V, I, V]
    L.harness_mist_transmittance.argtypes = [F, F, V, V, V, I, V]
    L.harness_mist_params.argtypes = [V, V, V]
    L.harness_mist_apply.argtypes = [V, I, I, V, V, I, V, I, V, V, V, V]
    return L


def options_of(opts=None):
    o = mist.mist_options(opts)
    if o is None:
        o = _lib.ow_mist_options()
        _lib.load().ow_mist_options_init(C.byref(o))
    return o


def values_of(o):
    """the option record as the twin reads it: FP32 values, slices resolved"""
    v = {k: (tuple(getattr(o, k)) if isinstance(getattr(o, k), C.Array) else getattr(o, k)) for k, _ in o._fields_ if k != "reserved"}
    v["slices"] = v["slices"] or 64
    return v


def cpu_apply(L, cam, records, opts=None, frame=None, size=0, words=None, skip=1):
    """the CPU build's pass: dict of rec (a copy, rewritten), A, B, S, ray, the counters and rgba.  frame: an _lib.ow_shadow_frame or None"""
    rec = np.array(records, W.RENDER_PIXEL, copy=True, order="C")
    assert rec.shape == (cam.height, cam.width)
    o = options_of(opts)
    cw = camera_words(cam)
    st = np.zeros((cam.height, cam.width, 10), np.float32)
    counters = np.zeros(3, np.uint64)
    rgba = np.zeros((cam.height, cam.width, 4), np.uint8)
    wd = np.ascontiguousarray(words, np.uint32) if words is not None else None
    L.harness_mist_apply(cw.ctypes.data, cam.width, cam.height, C.addressof(o), C.addressof(frame) if frame is not None else None, size,
                         wd.ctypes.data if wd is not None else None, skip, rec.ctypes.data, st.ctypes.data, counters.ctypes.data, rgba.ctypes.data)
    return dict(rec=rec, A=st[..., 0], B=st[..., 1], S=st[..., 2:5], ray=st[..., 5:8], slices_fetched=st[..., 8].astype(np.int64),
                slices_shadowed=st[..., 9].astype(np.int64), pixels=int(counters[0]), fetched=int(counters[1]),
                shadowed=int(counters[2]), rgba=rgba)


def cpu_cast(SL, frame, size, shape, tf, stride=12):
    """the shadows' CPU build (tests/shadow/): the depth words of one cast into a cleared map"""
    m, c = np.zeros((size, size), np.uint32), np.zeros(4, np.uint32)
    SL.harness_shadow_clear(size, m.ctypes.data, c.ctypes.data)
    v = np.ascontiguousarray(shape[0], np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(shape[1], np.int32).reshape(-1, 3)
    tf = np.ascontiguousarray(tf, np.float32)
    SL.harness_shadow_cast(C.addressof(frame), size, v.ctypes.data, len(v), t.ctypes.data, len(t), tf.ctypes.data if tf.size else None, stride, None,
                           tf.size // stride, m.ctypes.data, c.ctypes.data, None)
    return m


def ray_camera(position, direction, max_distance=4000.0):
    """a 1 x 1 camera whose only ray runs along `direction` (a unit vector) exactly: the pixel's ray is minus the basis' third column"""
    d = np.float64(direction)
    a = np.cross(d, [0.0, 1.0, 0.0]) if abs(d[1]) < 0.9 else np.cross(d, [1.0, 0.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(a, d)
    return W.camera(position, np.stack([a, b, -d], axis=1), 90.0, 1, 1, max_distance)


def one_record(t=None, color=(0.3, 0.5, 0.7), status=None):
    rec = np.zeros((1, 1), W.RENDER_PIXEL)
    rec["color"] = np.float32(color)
    rec["status"] = (HIT if t is not None else 0) if status is None else status
    rec["t"] = 0.0 if t is None else t
    rec["specular"], rec["reserved"] = 0.25, (1, 2, 3, 4)
    return rec


def horizontal(dy):
    return (float(np.sqrt(1.0 - dy * dy)), dy, 0.0)


def closed_form_cases():
    """(name, camera height, direction, record t or None, options): the rays of the closed form"""
    cases = []
    for dy in (0.0, 1e-7, -1e-7, 1.0, -1.0):
        d = horizontal(dy) if abs(dy) < 1 else (0.0, dy, 0.0)
        for y in (2.0, 0.0, -3.0):                                       # above the base, on it, a camera below it
            for t in (40.0, None):
                cases.append((f"dy {dy:g} from y {y:g} t {t}", y, d, t, {}))
    s = float(np.sqrt(1 - 0.3 ** 2))
    cases.append(("crosses the base from above", 5.0, (s, -0.3, 0.0), 100.0, {}))
    cases.append(("crosses the base from below", -4.0, (float(np.sqrt(1 - 0.25 ** 2)), 0.25, 0.0), 100.0, {}))
    cases.append(("crosses the base from above, no hit", 5.0, (s, -0.3, 0.0), None, {}))
    cases.append(("grazes down through the base", 1e-3, horizontal(-1e-4), 200.0, {}))
    cases.append(("a raised base", 2.0, horizontal(1e-7), 60.0, dict(base_height=1.5)))
    cases.append(("falloff 0", 4.0, (s, 0.3, 0.0), 35.0, dict(height_falloff=0.0)))
    cases.append(("a steep falloff", 0.5, (s, 0.3, 0.0), 35.0, dict(height_falloff=5.0, extinction=0.5)))
    cases.append(("a hit beyond length", 2.0, horizontal(0.0), 1000.0, {}))
    cases.append(("t = 0", 2.0, horizontal(0.0), 0.0, {}))
    cases.append(("thick mist", 1.0, horizontal(1e-7), None, dict(extinction=2.0)))
    return cases


def near_horizontal(d):
    return abs(d[1]) <= 1e-6


def margins():
    """name -> the largest difference measured (profiles/mist_margins.txt: lines `margin NAME VALUE`)"""
    out = {}
    for line in open(MARGINS):
        m = re.match(r"margin (\w+) ([0-9.e+-]+)", line)
        if m:
            out[m.group(1)] = float(m.group(2))
    return out


# ---- 1. the interface and the documents --------------------------------------------------------------------------------------------------

def test_header_declares_the_new_calls_and_the_library_exports_them():
    build.build_library()
    lib = _lib.load()
    check_declared_and_bound(lib, NEW_FUNCTIONS)
    assert sorted(s for s in exported_symbols() if "mist" in s) == sorted(NEW_FUNCTIONS)          # no group form, no handle: no destroy
    for define, value in (("OW_RAY_MIST", 256), ("OW_MIST_MAX_SLICES", 256)):
        assert re.search(r"#define %s %d\b" % (define, value), HEADER) and getattr(_lib, define) == value, define
    section = HEADER.split("Height mist with sun shafts")[1].split("several devices")[0]
    for cite in ("water -> solids -> ow_shadow_apply -> ow_radiance_light_apply -> ow_environment_apply -> ow_mist_apply -> billboards -> ow_present",
                 "ow_mist.h", "THIS LIBRARY'S CHOICE", "main.tscn:35-37", ":100-104", ":142-144", "main.tscn:113", "main.tscn:101", "height_falloff = 0.176",
                 "OW_RAY_MIST", "no group form", "local fog volumes, density textures, temporal reprojection, light from the sky in the mist",
                 "not fogged", "SUBTRACTED"):
        assert cite in section, cite
    assert "Shadowed fog scatter is ow_mist_apply's" in HEADER.split("Sun shadows of the floating bodies")[1].split("Height mist")[0]
    assert "they are ow_mist_apply's" in HEADER.split("ow_environment_options")[0]
    note = open(os.path.join(CSRC, "ow_mist.h")).read()
    for cite in ("THIS LIBRARY'S CHOICE", "-ffp-contract=off", "LENGTH x MEAN WEIGHT", "mist_span"):
        assert cite in note, cite
    o = _lib.ow_mist_options()
    lib.ow_mist_options_init(C.byref(o))
    f = lambda v: float(np.float32(v))     # noqa: E731
    assert (o.height_falloff, o.length, o.base_height, o.anisotropy, o.sky_affect) == (f(0.176), 256.0, 0.0, f(0.2), 1.0)
    assert list(o.albedo) == [f(0.988718), f(0.989631), f(0.989629)] and np.allclose(list(o.sun_direction), SUN, rtol=0, atol=1e-6)   # main.tscn:113
    assert 0.0 < o.extinction <= 1.0 and (o.slices, o.flags, o.shadow_bias) == (64, 0, 0.0) and not any(o.reserved)
    assert list(o.sun_color) == [1.0, 1.0, 1.0]
    lib.ow_mist_options_init(None)


def test_structs_agree_in_c_ctypes_and_the_harness(tmp_path, harness):
    name, St = "ow_mist_options", _lib.ow_mist_options
    fields = [f for f, _ in St._fields_]
    expr = ", ".join(["sizeof(%s)" % name] + ["offsetof(%s, %s)" % (name, f) for f in fields])
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ocean_waves.h"\nint main(void){printf("%s\\n", ' % " ".join(["%zu"] * (1 + len(fields)))
           + expr + ");return 0;}\n")
    vals = layout_probe(tmp_path, name + "_layout", src)
    assert vals == [C.sizeof(St)] + [getattr(St, f).offset for f in fields] and vals[0] == 128
    assert vals[1:] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 48, 60, 72, 84]
    sizes = (C.c_int * 16)()
    harness.harness_mist_sizes(sizes)
    assert list(sizes) == [128] + vals[2:] + [MIST, _lib.OW_MIST_MAX_SLICES]
    assert CASE.itemsize == 16 + 60 + 4 + 128 + 64


def test_the_documents_name_the_new_calls():
    for name in NEW_FUNCTIONS:
        assert "`%s`" % name in S.DOC.split("## 7. Index")[1], name
    for name in NEW_FUNCTIONS[1:]:
        assert re.search(r"\[DllImport\(Lib\)\]\s*public static extern \w+ %s\(" % name, S.SHIM), name
    order = "water -> solids -> ow_shadow_apply -> ow_radiance_light_apply -> ow_environment_apply -> ow_mist_apply -> billboards -> ow_present"
    for doc, words in (("README.md", ("ow_mist_apply", "profiles/mist_1024x4.txt")),
                       ("DESIGN.md", ("k_mist_apply", "ow_mist.hip", "ow_mist.h", "mist_span")),
                       ("INTEGRATION.md", ("ow_mist_apply_async", "OW_RAY_MIST", "OwMistOptions", order))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)
    for path in ("scripts/mist_cost.py", "examples/mist_host.c", "profiles/mist_kernels_isa.txt", "profiles/mist_margins.txt"):
        assert os.path.exists(os.path.join(ROOT, path)), path


def test_example_builds_as_c99(tmp_path):
    build.build_library()
    build_example(tmp_path, "mist_host")


# ---- 2. argument errors without a device ---------------------------------------------------------------------------------------------------

def test_argument_errors_without_a_device():
    lib = _lib.load()
    cam = level_camera(24, 12)
    rec = np.zeros((12, 24), W.RENDER_PIXEL)
    rgba = np.zeros((12, 24, 4), np.uint8)
    fake = C.c_void_p(16)   # never read: every case fails before a handle is looked at

    def apply(camera, opts, rec_p=rec.ctypes.data, shadow_map=fake):
        cp, op = (C.byref(camera) if camera is not None else None), (C.byref(opts) if opts is not None else None)
        out = []
        for fn in (lib.ow_mist_apply, lib.ow_mist_apply_async):
            assert fn(None, shadow_map, cp, op, rec_p, rgba.ctypes.data) == _lib.OW_ERR_INVALID
            out.append(lib.ow_last_error().decode())
        assert out[0] == out[1]
        return out[0]

    mo = mist.mist_options
    assert "null context" in apply(cam, None) and "null context" in apply(cam, None, shadow_map=None)       # everything else is in order
    assert "null context" in apply(cam, mo(dict(extinction=1e3, height_falloff=1e3, anisotropy=-0.9, sky_affect=0.0, slices=256, length=0.0)))
    assert "null context" in apply(cam, mo(dict(extinction=0.0, height_falloff=0.0, anisotropy=0.9, slices=1)))
    assert "the records" in apply(cam, None, None)
    assert "null camera" in apply(None, None)
    for w, h in ((0, 12), (24, 0), (_lib.OW_RENDER_MAX_SIDE + 1, 12)):
        assert "camera size" in apply(level_camera(w, h), None)
    bad = level_camera(24, 12)
    bad.reserved[1] = 7
    assert "ow_camera.reserved" in apply(bad, None)
    nan, inf = float("nan"), float("inf")
    for key, values in (("extinction", (nan, inf, -1e-3, 2e3)), ("height_falloff", (nan, -1.0, 2e3)), ("base_height", (nan, inf, -2e6)),
                        ("length", (nan, -1.0, 2e6)), ("anisotropy", (nan, 0.95, -0.95)), ("sky_affect", (nan, -0.1, 1.1)),
                        ("shadow_bias", (nan, inf, 2e6))):
        for v in values:
            assert key in apply(cam, mo({key: v})), (key, v)
    for n in (-1, 257):
        assert "slices" in apply(cam, mo(dict(slices=n))), n
    for key in ("albedo", "sun_color", "ambient_color"):
        for v in ((nan, 0, 0), (0, -1, 0), (0, 0, inf)):
            assert "colour" in apply(cam, mo({key: v})), (key, v)
    assert "sun_direction" in apply(cam, mo(dict(sun_direction=(0, nan, 1)))) and "zero length" in apply(cam, mo(dict(sun_direction=(0, 0, 0))))
    # the order: the records before the camera before the options
    assert "the records" in apply(None, mo(dict(sky_affect=2.0)), None) and "null camera" in apply(None, mo(dict(sky_affect=2.0)))
    o = mo({})
    o.flags = 1
    assert "unknown mist flags" in apply(cam, o)
    o = mo({})
    o.reserved[10] = 1
    assert "ow_mist_options.reserved" in apply(cam, o)
    assert lib.ow_mist_stats(None, None, None, None, None) == _lib.OW_ERR_INVALID and "null context" in lib.ow_last_error().decode()
    assert not rec.tobytes().strip(b"\0") and not rgba.any()
    with pytest.raises(ValueError):
        mo(dict(density=1.0))


# ---- 3. the closed form ------------------------------------------------------------------------------------------------------------------------

def measure_closed_form(harness):
    """the largest |A - twin|, |color - twin| over the closed form's cases, apart for the near-horizontal rays and the others"""
    worst = dict(steep=0.0, level=0.0)
    for name, y, d, t, extra in closed_form_cases():
        cam = ray_camera((1.0, y, -2.0), d)
        rec = one_record(t)
        got = cpu_apply(harness, cam, rec, extra)
        want = MT.apply(camera_words(cam), rec, values_of(options_of(extra)))
        assert np.abs(got["ray"][0, 0] - np.float32(d)).max() == 0.0, name                  # the ray is the one asked for, to the bit
        assert got["rec"]["status"][0, 0] == rec["status"][0, 0] | MIST and got["B"][0, 0] == 0.0, name
        e = max(float(np.abs(got["A"] - want["A"]).max()), float(np.abs(got["rec"]["color"] - want["color"]).max()))
        print(f"{name}: A {float(got['A'][0, 0]):.7g} twin {float(want['A'][0, 0]):.7g} error {e:.3e}")
        key = "level" if near_horizontal(d) else "steep"
        worst[key] = max(worst[key], e)
    return worst


def test_closed_form_against_the_fp64_twin(harness):
    """Measured on the CPU build (profiles/mist_margins.txt; the figures go to the file with MIST_WRITE_MARGINS=1): the largest differences of A
    and of the colour from the twin over the cases, four times which is allowed; the near-horizontal rays (|d.y| <= 1e-6) stay within the
    same margin as the steep ones"""
    worst = measure_closed_form(harness)
    print(worst)
    if os.environ.get("MIST_WRITE_MARGINS") == "1":
        return
    allowed = 4.0 * margins()["closed_form"]
    assert worst["steep"] <= allowed and worst["level"] <= allowed, (worst, allowed)
    assert allowed <= 4e-6                       # a few ulp of values of order one: what FP32 gives, not a tolerance opened up


def test_closed_form_limits(harness):
    s = float(np.sqrt(1 - 0.3 ** 2))
    m = 4.0 * margins()["closed_form"]
    cam = ray_camera((0.0, 4.0, 0.0), (s, 0.3, 0.0))
    flat = cpu_apply(harness, cam, one_record(35.0), dict(height_falloff=0.0, extinction=0.05))       # falloff 0: T = exp(-extinction t)
    assert abs(float(flat["A"][0, 0]) - (1.0 - np.exp(-float(np.float32(0.05)) * 35.0))) <= m
    rec = one_record(35.0)
    clear = cpu_apply(harness, cam, rec, dict(extinction=0.0))["rec"]                                 # extinction 0: only status changes
    for f in W.RENDER_PIXEL.names:
        assert (clear[f].tobytes() == rec[f].tobytes()) == (f != "status"), f
    assert clear["status"][0, 0] == HIT | MIST
    level = ray_camera((0.0, 2.0, 0.0), horizontal(0.0))
    far = cpu_apply(harness, level, one_record(1000.0))                                               # a hit beyond length stops at length
    at = cpu_apply(harness, level, one_record(256.0))
    assert far["rec"]["color"].tobytes() == at["rec"]["color"].tobytes() and far["A"][0, 0] == at["A"][0, 0] > 0.5
    zero = cpu_apply(harness, level, one_record(0.0))                                                 # t = 0: no mist in front of the hit
    assert zero["A"][0, 0] == 0.0 and zero["rec"]["color"].tobytes() == one_record(0.0)["color"].tobytes()
    below = cpu_apply(harness, ray_camera((0.0, -3.0, 0.0), horizontal(0.0)), one_record(40.0), dict(extinction=0.03))   # all of it below the base
    assert abs(float(below["A"][0, 0]) - (1.0 - np.exp(-float(np.float32(0.03)) * 40.0))) <= m
    x = np.float32([0.0, 1e-8, 1e-3, 0.25, 0.499999, 0.5, 0.500001, 1.0, 10.0, 100.0, 1e6])             # phi: its series, its switch, its tail
    got = np.zeros_like(x)
    harness.harness_mist_phi(x.ctypes.data, len(x), got.ctypes.data)
    assert np.abs(got - MT.phi(x.astype(np.float64))).max() <= 2.5e-7 and got[0] == 1.0


def test_near_horizontal_rays_do_not_cancel(harness):
    """T over a sweep of slopes from 1e-9 to 1 through a camera above, on and below the base: one margin for all of them"""
    slopes = np.concatenate([[0.0], np.logspace(-9, 0, 37)])
    dy = np.concatenate([slopes, -slopes]).astype(np.float32)
    worst = 0.0
    for h0 in (2.0, 0.0, -3.0, 1e-4):
        for t in (40.0, 256.0):
            h = np.full_like(dy, h0)
            tt = np.full_like(dy, t)
            got = np.zeros_like(dy)
            k = float(np.float32(0.176 * MT.LN2))
            harness.harness_mist_transmittance(0.02, k, h.ctypes.data, dy.ctypes.data, tt.ctypes.data, len(dy), got.ctypes.data)
            want = MT.transmittance(float(np.float32(0.02)), k, h.astype(np.float64), dy.astype(np.float64), tt.astype(np.float64))
            worst = max(worst, float(np.abs(got - want).max()))
    print(f"worst |T - twin| over the sweep {worst:.3e}")
    assert worst <= 4.0 * margins()["closed_form"]


# ---- 4. the shafts -------------------------------------------------------------------------------------------------------------------------

SHAFT_FRAME = dict(light_direction=SUN, half_extent=14.0, center=(0.0, 1.0, 4.0), depth_range=40.0)
SHAFT_SIZE = 64
SHAFT_CAM = dict(position=(-13.0, 2.5, 3.0), yaw_deg=88.0, pitch_deg=-3.0, fov=60.0, width=48, height=32, max_distance=500.0)
SHAFT_OPTS = dict(length=40.0, extinction=0.05)
CRATE = transforms([((0.0, 1.6, 9.0), (0.0, 0.0, 0.0, 1.0), 2.5)])


def shaft_scene(shadow_harness):
    fr = W.shadow_frame(SHAFT_FRAME)
    words = cpu_cast(shadow_harness, fr, SHAFT_SIZE, cube(), CRATE)
    assert (words != FLT_MAX_BITS).sum() > 30
    cam = look(**SHAFT_CAM)
    rec = np.zeros((cam.height, cam.width), W.RENDER_PIXEL)
    rec["color"] = (0.2, 0.3, 0.4)
    rec["status"][:, ::2] = HIT                           # every other column stops at 30 m, the others run the mist's whole length
    rec["t"][:, ::2] = 30.0
    return fr, words, cam, rec


def shaft_twin(fr, words, cam, rec, opts):
    tf = ST.frame(SHAFT_FRAME["light_direction"], SHAFT_FRAME["half_extent"], SHAFT_FRAME["center"], SHAFT_FRAME["depth_range"], SHAFT_SIZE)
    return MT.apply(camera_words(cam), rec, values_of(options_of(opts)), tf, words.view(np.float32))


def measure_shafts(harness, shadow_harness):
    fr, words, cam, rec = shaft_scene(shadow_harness)
    got = cpu_apply(harness, cam, rec, SHAFT_OPTS, fr, SHAFT_SIZE, words)
    want = shaft_twin(fr, words, cam, rec, SHAFT_OPTS)
    keep = ~want["ambiguous"]
    share = 1.0 - keep.mean()
    behind = keep & (want["shadowed"] > 0)
    e = dict(B=float(np.abs(got["B"] - want["B"])[keep].max()), color=float(np.abs(got["rec"]["color"] - want["color"])[keep].max()))
    return got, want, keep, behind, share, e


def test_the_twin_alone_keeps_the_shaft_scene_unambiguous(shadow_harness):
    fr, words, cam, rec = shaft_scene(shadow_harness)
    want = shaft_twin(fr, words, cam, rec, SHAFT_OPTS)
    share = float(want["ambiguous"].mean())
    print(f"ambiguous {share:.4f}, pixels behind the crate {int((want['shadowed'] > 0).sum())}")
    assert share <= 0.02 and (want["shadowed"] > 0).sum() >= 100 and (want["shadowed"] == 0).sum() >= 100


def test_rays_behind_one_crate_lose_the_twins_share(harness, shadow_harness):
    """one crate on a 64^2 map, 48 x 32 rays across its shaft: the slices found shadowed are the twin's, B and the colour within four times
    the differences recorded in profiles/mist_margins.txt, at most 2 % of the pixels set aside"""
    got, want, keep, behind, share, e = measure_shafts(harness, shadow_harness)
    print(f"set aside {share:.4f}, behind the crate {int(behind.sum())}, largest B {float(want['B'].max()):.4f}", e)
    assert share <= 0.02 and behind.sum() >= 100
    assert np.array_equal(got["slices_shadowed"][keep], want["shadowed"][keep]) and got["slices_shadowed"].sum() == got["shadowed"]
    assert ((got["B"] > 0) == (want["B"] > 0))[keep].all() and float(want["B"][behind].max()) > 0.05
    assert (got["B"][keep & (want["shadowed"] == 0)] == 0.0).all()
    if os.environ.get("MIST_WRITE_MARGINS") == "1":
        return
    m = margins()
    assert e["B"] <= 4.0 * m["shafts_B"] and e["color"] <= 4.0 * m["shafts_color"], (e, m)
    assert 4.0 * m["shafts_B"] <= 2e-5
    lit = cpu_apply(harness, look(**SHAFT_CAM), shaft_scene(shadow_harness)[3], SHAFT_OPTS)
    darker = (got["rec"]["color"] < lit["rec"]["color"]).all(-1)
    assert np.array_equal(darker[keep], (want["B"] > 0)[keep])                     # a shaft only ever takes light away


def test_write_margins(harness, shadow_harness):
    """with MIST_WRITE_MARGINS=1: measures and writes profiles/mist_margins.txt; otherwise holds the file to its form"""
    if os.environ.get("MIST_WRITE_MARGINS") == "1":
        worst = measure_closed_form(harness)
        _, want, keep, behind, share, e = measure_shafts(harness, shadow_harness)
        with open(MARGINS, "w") as out:
            out.write("# The height mist's CPU build (tests/mist/mist_harness.cpp) against the FP64 twin (tests/mist_twin.py), written by\n"
                      "# tests/test_mist.py::test_write_margins with MIST_WRITE_MARGINS=1.  The tests assert four times each value of a `margin` line.\n"
                      "# closed_form: the largest |A - twin| and |color - twin| over the closed form's cases (1 x 1 pictures whose ray is given exactly:\n"
                      "# d.y = 0, +-1e-7, +-1 from above, on and below the base, rays that cross the base both ways, falloff 0, a steep falloff, a hit\n"
                      "# beyond length, t = 0, thick mist), colours of order one.  steep / level: the same apart for the rays with |d.y| > 1e-6 and\n"
                      "# the near-horizontal ones -- the mean-weight form keeps them alike.\n")
            out.write(f"margin closed_form {max(worst.values()):.3e}\n")
            out.write(f"measured steep {worst['steep']:.3e} level {worst['level']:.3e} allowed {4 * max(worst.values()):.3e}\n")
            out.write("# shafts: one 2.5 m crate on a 64^2 map, 48 x 32 rays across its shaft, 64 slices, length 40, extinction 0.05; a pixel with a\n"
                      "# depth compare within 1e-4 m of flipping in the twin is set aside (the test allows 2 %).\n")
            out.write(f"shafts set aside {share:.4f} behind the crate {int(behind.sum())} largest B {float(want['B'].max()):.4f}\n")
            out.write(f"margin shafts_B {e['B']:.3e}\nmargin shafts_color {e['color']:.3e}\n")
    m = margins()
    assert set(m) == {"closed_form", "shafts_B", "shafts_color"} and all(0.0 < v <= 5e-6 for v in m.values()), m
    text = open(MARGINS).read()
    assert float(re.search(r"set aside ([0-9.]+)", text).group(1)) <= 0.02


# ---- 5. bit identities -------------------------------------------------------------------------------------------------------------------------

def identity_records(cam, seed=3):
    rec = synthetic_records(cam, seed=seed, top=4.0)
    rec["t"] = np.where(rec["t"] > 0, np.minimum(rec["t"], 80.0), rec["t"])
    return rec


def test_maps_that_shadow_nothing_give_the_same_bytes(harness, shadow_harness):
    fr, words, cam, _ = shaft_scene(shadow_harness)
    rec = identity_records(cam)
    none = cpu_apply(harness, cam, rec, SHAFT_OPTS)
    assert none["fetched"] == 0 and none["shadowed"] == 0 and none["pixels"] == rec.size
    dead = _lib.ow_shadow_frame()                                                  # all zeros: what a map holds before its first begin
    never = cpu_apply(harness, cam, rec, SHAFT_OPTS, dead, SHAFT_SIZE, words)
    empty = cpu_apply(harness, cam, rec, SHAFT_OPTS, fr, SHAFT_SIZE, np.full((SHAFT_SIZE, SHAFT_SIZE), FLT_MAX_BITS, np.uint32))
    aside = cpu_cast(shadow_harness, fr, SHAFT_SIZE, cube(), transforms([((-5.0, -8.0, -8.0), (0, 0, 0, 1), 1.0)]))   # below and behind every ray
    assert (aside != FLT_MAX_BITS).any()
    away = cpu_apply(harness, cam, rec, SHAFT_OPTS, fr, SHAFT_SIZE, aside)
    assert empty["fetched"] > 1000 and away["fetched"] == empty["fetched"] and away["shadowed"] == 0
    for other in (never, empty, away):
        assert other["rec"].tobytes() == none["rec"].tobytes() and other["rgba"].tobytes() == none["rgba"].tobytes()
    real = cpu_apply(harness, cam, rec, SHAFT_OPTS, fr, SHAFT_SIZE, words)
    assert real["shadowed"] > 100 and real["rec"].tobytes() != none["rec"].tobytes()


def test_twice_is_once_and_only_color_and_status_change(harness, shadow_harness):
    fr, words, cam, _ = shaft_scene(shadow_harness)
    rec = identity_records(cam)
    once = cpu_apply(harness, cam, rec, SHAFT_OPTS, fr, SHAFT_SIZE, words)
    twice = cpu_apply(harness, cam, once["rec"], SHAFT_OPTS, fr, SHAFT_SIZE, words)
    assert twice["rec"].tobytes() == once["rec"].tobytes() and twice["pixels"] == 0
    for f in W.RENDER_PIXEL.names:
        if f not in ("status", "color"):
            assert once["rec"][f].tobytes() == rec[f].tobytes(), f
    assert (once["rec"]["status"] == (rec["status"] | MIST)).all() and (once["rec"]["color"] != rec["color"]).any()
    part = rec.copy()
    part["status"][::2] |= MIST                                                   # rows that carry the flag already are left alone
    got = cpu_apply(harness, cam, part, SHAFT_OPTS, fr, SHAFT_SIZE, words)
    assert got["rec"][::2].tobytes() == part[::2].tobytes() and got["rec"][1::2].tobytes() == once["rec"][1::2].tobytes()
    assert np.array_equal(once["rgba"], _rgba8(once["rec"]["color"]))


def _rgba8(color):
    c = np.asarray(color, np.float32)
    v = np.where(c > 0, np.where(c < 1, c, np.float32(1)), np.float32(0))
    out = np.full(c.shape[:-1] + (4,), 255, np.uint8)
    out[..., :3] = (v * np.float32(255) + np.float32(0.5)).astype(np.uint8)
    return out


def test_slices_0_is_64_and_skipping_lit_slices_changes_no_bit(harness, shadow_harness):
    fr, words, cam, _ = shaft_scene(shadow_harness)
    rec = identity_records(cam)
    a = cpu_apply(harness, cam, rec, dict(SHAFT_OPTS, slices=0), fr, SHAFT_SIZE, words)
    b = cpu_apply(harness, cam, rec, dict(SHAFT_OPTS, slices=64), fr, SHAFT_SIZE, words)
    assert a["rec"].tobytes() == b["rec"].tobytes() and (a["fetched"], a["shadowed"]) == (b["fetched"], b["shadowed"])
    rng = np.random.default_rng(8)
    for k in range(12):                                   # frames small and large, beside, behind and around the camera; every slice count's kind
        frame = W.shadow_frame(dict(light_direction=tuple(rng.normal(size=3)), half_extent=float(rng.choice([0.5, 6.0, 14.0, 300.0])),
                                    center=tuple(rng.uniform(-20, 20, 3)), depth_range=float(rng.choice([2.0, 40.0, 500.0]))))
        size = int(rng.choice([8, 33, 64]))
        noise = np.where(rng.random((size, size)) < 0.5, np.float32(rng.uniform(0, 60, (size, size))).view(np.uint32), np.uint32(FLT_MAX_BITS)).astype(np.uint32)
        c = look(position=tuple(rng.uniform(-15, 15, 3)), yaw_deg=float(rng.uniform(0, 360)), pitch_deg=float(rng.uniform(-60, 60)), fov=70.0, width=19, height=13)
        o = dict(length=float(rng.choice([5.0, 60.0, 1000.0])), slices=int(rng.choice([1, 7, 64, 256])), shadow_bias=float(rng.uniform(-2, 2)))
        r = identity_records(c, seed=k)
        every = cpu_apply(harness, c, r, o, frame, size, noise, skip=0)
        fewer = cpu_apply(harness, c, r, o, frame, size, noise, skip=1)
        assert fewer["rec"].tobytes() == every["rec"].tobytes() and (fewer["fetched"], fewer["shadowed"]) == (every["fetched"], every["shadowed"]), k
        assert fewer["B"].tobytes() == every["B"].tobytes()


# ---- 6. sizes and edges --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width,height", [(1, 1), (8, 8), (19, 13)])
@pytest.mark.parametrize("slices", [1, 256])
def test_sizes_and_slice_counts_against_the_twin(harness, shadow_harness, width, height, slices):
    fr, words, _, _ = shaft_scene(shadow_harness)
    cam = look(**dict(SHAFT_CAM, width=width, height=height))
    rec = identity_records(cam, seed=width)
    opts = dict(SHAFT_OPTS, slices=slices)
    got = cpu_apply(harness, cam, rec, opts, fr, SHAFT_SIZE, words)
    want = shaft_twin(fr, words, cam, rec, opts)
    keep = ~want["ambiguous"]
    m = margins()
    assert got["pixels"] == width * height and np.array_equal(got["rec"]["status"], want["status"])
    assert np.abs(got["A"] - want["A"]).max() <= 4.0 * m["closed_form"]
    scale = np.maximum(1.0, np.abs(want["color"]))
    if keep.any():
        assert (np.abs(got["B"] - want["B"])[keep]).max() <= 4.0 * m["shafts_B"] * max(1.0, slices / 64.0)
        assert (np.abs(got["rec"]["color"] - want["color"]) / scale)[keep].max() <= 4.0 * m["shafts_color"] * max(1.0, slices / 64.0)


def test_sky_affect_a_nan_colour_and_a_camera_that_is_not_finite(harness):
    cam = look(**dict(SHAFT_CAM, width=19, height=13))
    rec = identity_records(cam)
    none = cpu_apply(harness, cam, rec, dict(sky_affect=0.0))
    miss = (rec["status"] & HIT) == 0
    assert miss.sum() > 20 and (none["rec"]["status"] == (rec["status"] | MIST)).all()
    assert none["rec"]["color"][miss].tobytes() == rec["color"][miss].tobytes()            # marked, the colour unchanged
    full = cpu_apply(harness, cam, rec, dict(sky_affect=1.0))
    assert (full["rec"]["color"][miss] != rec["color"][miss]).any()
    assert full["rec"][~miss].tobytes() == none["rec"][~miss].tobytes()                     # sky_affect is the misses' alone
    half = cpu_apply(harness, cam, rec, dict(sky_affect=0.5))
    want = MT.apply(camera_words(cam), rec, values_of(options_of(dict(sky_affect=0.5))))
    assert (np.abs(half["rec"]["color"] - want["color"]) / np.maximum(1.0, np.abs(want["color"]))).max() <= 4.0 * margins()["shafts_color"]
    odd = rec.copy()
    odd["color"][2, 3] = (np.nan, 0.5, np.inf)
    odd["color"][4, 5] = (-np.inf, np.nan, 3e38)
    got = cpu_apply(harness, cam, odd)
    assert np.isfinite(got["rec"]["color"]).all()
    for (j, i), ks in (((2, 3), (0, 2)), ((4, 5), (0, 1))):
        for k in ks:
            assert got["rec"]["color"][j, i, k] == got["S"][j, i, k]                         # a channel that is not finite takes S
    dead = look(**dict(SHAFT_CAM, width=19, height=13))
    dead.position[1] = float("nan")
    same = cpu_apply(harness, dead, rec)
    assert same["rec"].tobytes() == rec.tobytes() and same["pixels"] == 0                    # every byte as it was
    dead = look(**dict(SHAFT_CAM, width=19, height=13))
    dead.basis[4] = float("inf")
    assert cpu_apply(harness, dead, rec)["rec"].tobytes() == rec.tobytes()


def fuzz_case(rng, k):
    big = k % 3 == 0
    pick = lambda lo, hi: float(rng.choice([lo, hi, rng.uniform(lo, hi)]))    # noqa: E731
    col = lambda top: tuple(float(x) for x in rng.choice([0.0, top, rng.uniform(0, top)], 3))    # noqa: E731
    top = 1e6 if big else 2.0
    o = dict(extinction=pick(0.0, 1e3 if big else 0.2), height_falloff=pick(0.0, 1e3 if big else 1.0), base_height=pick(-1e6, 1e6) if big else pick(-5, 5),
             length=pick(0.0, 1e6 if big else 300.0), anisotropy=pick(-0.9, 0.9), sky_affect=pick(0.0, 1.0), slices=int(rng.choice([0, 1, 13, 256])),
             shadow_bias=pick(-1e6, 1e6) if big else pick(-3, 3), albedo=col(top), sun_color=col(top), ambient_color=col(top),
             sun_direction=tuple(float(x) for x in rng.normal(size=3) * rng.choice([1e-6, 1.0, 1e5])))
    pos = tuple(rng.uniform(-1e6, 1e6, 3)) if big else tuple(rng.uniform(-20, 20, 3))
    cam = look(position=pos, yaw_deg=float(rng.uniform(0, 360)), pitch_deg=float(rng.choice([-89.9, 0.0, 89.9, rng.uniform(-89, 89)])), fov=float(rng.uniform(1, 170)),
               width=11, height=7)
    rec = synthetic_records(cam, seed=k, top=1e30 if big else 10.0)
    rec["t"].flat[::5] = rng.choice(np.float32([np.nan, np.inf, -np.inf, -1.0, 3e38, 1e-30]), rec["t"].flat[::5].shape)
    rec["color"].flat[::7] = rng.choice(np.float32([np.nan, np.inf, -np.inf, 3.4e38, -3.4e38]), rec["color"].flat[::7].shape)
    frame = W.shadow_frame(dict(light_direction=tuple(rng.normal(size=3)), half_extent=float(rng.choice([1e-3, 10.0, 1e6])), center=pos,
                                depth_range=float(rng.choice([1e-3, 40.0, 1e6]))))
    size = int(rng.choice([8, 64]))
    words = np.where(rng.random((size, size)) < 0.5, np.float32(rng.uniform(0, 80, (size, size))).view(np.uint32), np.uint32(FLT_MAX_BITS)).astype(np.uint32)
    return cam, rec, o, frame, size, words


def test_no_nan_or_inf_comes_out_of_fuzzed_finite_options(harness):
    rng = np.random.default_rng(20261020)
    for k in range(60):
        cam, rec, o, frame, size, words = fuzz_case(rng, k)
        got = cpu_apply(harness, cam, rec, o, frame, size, words)
        assert np.isfinite(got["rec"]["color"]).all() and np.isfinite(got["A"]).all() and np.isfinite(got["B"]).all() and np.isfinite(got["S"]).all(), (k, o)
        assert (got["A"] >= 0).all() and (got["A"] <= 1).all() and (got["B"] >= 0).all() and (got["B"] <= got["A"]).all(), k
        every = cpu_apply(harness, cam, rec, o, frame, size, words, skip=0)
        assert every["rec"].tobytes() == got["rec"].tobytes() and every["fetched"] == got["fetched"], k
        for f in W.RENDER_PIXEL.names:
            if f not in ("status", "color"):
                assert got["rec"][f].tobytes() == rec[f].tobytes(), f


# ---- 7. the sanitizers ---------------------------------------------------------------------------------------------------------------------

def write_case(path, cam, rec, opts, frame, size, words):
    h = np.zeros(1, CASE)
    h["width"], h["height"], h["size"], h["has_map"], h["cam"] = cam.width, cam.height, size, int(words is not None), camera_words(cam)
    h["options"] = np.frombuffer(bytes(options_of(opts)), np.uint8)
    if frame is not None:
        h["frame"] = np.frombuffer(bytes(frame), np.uint8)
    with open(path, "wb") as f:
        for block in (h,) + ((np.ascontiguousarray(words, np.uint32),) if words is not None else ()) + (np.ascontiguousarray(rec),):
            f.write(block.tobytes())


def test_stand_alone_harness_runs_clean_under_the_sanitizers(tmp_path, harness, shadow_harness):
    """the harness as a program of its own (-DMIST_HARNESS_MAIN), built with -fsanitize=address,undefined, on the shaft scene, a picture
    without a map and twelve fuzzed cases: what it writes is the shared library's, byte for byte, with the skip and without"""
    exe = build_sanitized_harness("mist", tmp_path)
    fr, words, cam, rec = shaft_scene(shadow_harness)
    cases = [(cam, rec, SHAFT_OPTS, fr, SHAFT_SIZE, words), (cam, identity_records(cam), dict(slices=256), None, 0, None)]
    rng = np.random.default_rng(5)
    cases += [fuzz_case(rng, k) for k in range(12)]
    for k, (c, r, o, frame, size, wd) in enumerate(cases):
        path, out = str(tmp_path / f"case{k}.bin"), str(tmp_path / f"case{k}.out")
        write_case(path, c, r, o, frame, size, wd)
        p = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (k, p.stdout + p.stderr)
        assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (k, p.stderr)
        want = b""
        for skip in (0, 1):
            g = cpu_apply(harness, c, r, o, frame, size, wd, skip=skip)
            st = np.concatenate([g["A"][..., None], g["B"][..., None], g["S"], g["ray"], g["slices_fetched"][..., None], g["slices_shadowed"][..., None]],
                                -1).astype(np.float32)
            want += g["rec"].tobytes() + st.tobytes() + np.uint64([g["pixels"], g["fetched"], g["shadowed"]]).tobytes() + g["rgba"].tobytes()
        assert open(out, "rb").read() == want, k


# ---- 8. on the GPU -------------------------------------------------------------------------------------------------------------------------

GPU_FRAME = dict(center=(0.3, 0.0, 8.5), half_extent=16.0, depth_range=40.0)
GPU_CAM = dict(position=(-15.0, 2.0, 4.0), yaw_deg=80.0, pitch_deg=-2.0, fov=70.0, max_distance=2000.0)
GPU_OPTS = dict(length=60.0, extinction=0.04)


def gpu_scene():
    """256^2 x 1 maps, eight crates never stepped (the poses of ow_bodies_create), the first three cast into a 64^2 map from the scene's sun"""
    gen, params = make_gen(256, [0])
    st, hull = eight_crates()
    bodies = gen.bodies_create(st, hull)
    solid = gen.solid_create(*box(CRATE_SHAPE))
    shadow = gen.shadow_map_create(64)
    gen.shadow_map_begin(shadow, GPU_FRAME)
    gen.shadow_map_cast(shadow, solid, bodies, first=0, count=3)
    return gen, params, bodies, solid, shadow


def close_scene(gen, bodies, solid, shadow):
    gen.shadow_map_destroy(shadow)
    gen.solid_destroy(solid)
    gen.bodies_destroy(bodies)
    gen.free()


@pytest.mark.gpu
@pytest.mark.parametrize("width,height", [(19, 13), (64, 40)])
def test_gpu_pass_is_the_cpu_builds_bit_for_bit(harness, width, height):
    """ragged tiles and whole ones; with the map, without one and with a map never begun; with and without the RGBA8 words; 1, 64 and 256
    slices; the counters are the CPU build's"""
    gen, params, bodies, solid, shadow = gpu_scene()
    words = gen.shadow_map_read(shadow).view(np.uint32)
    assert (words != FLT_MAX_BITS).sum() > 10
    fr = W.shadow_frame(GPU_FRAME)
    cam = look(**dict(GPU_CAM, width=width, height=height))
    rec = identity_records(cam, seed=height)
    shafts = 0
    for slices in (1, 64, 256):
        opts = dict(GPU_OPTS, slices=slices, shadow_bias=0.25)
        want = cpu_apply(harness, cam, rec, opts, fr, 64, words)
        for rgba in (True, False):
            img, out = mist.mist_apply(gen, cam, rec, shadow, opts, rgba=rgba)
            assert out.tobytes() == want["rec"].tobytes(), (slices, rgba)
            assert (img is None) if not rgba else (img.tobytes() == want["rgba"].tobytes()), slices
        st = mist.mist_stats(gen)
        assert (st["pixels"], st["slices_fetched"], st["slices_shadowed"]) == (want["pixels"], want["fetched"], want["shadowed"]), slices
        shafts += want["shadowed"]
    assert shafts > 50                                                             # the crates' shafts are in the picture
    bare = cpu_apply(harness, cam, rec, GPU_OPTS)
    img, out = mist.mist_apply(gen, cam, rec, None, GPU_OPTS, rgba=True)
    assert out.tobytes() == bare["rec"].tobytes() and img.tobytes() == bare["rgba"].tobytes()
    st = mist.mist_stats(gen)
    assert (st["pixels"], st["slices_fetched"], st["slices_shadowed"]) == (rec.size, 0, 0)   # without a map nothing is fetched
    fresh = gen.shadow_map_create(16)                                              # a map that has had no begin: likewise
    _, out = mist.mist_apply(gen, cam, rec, fresh, GPU_OPTS)
    assert out.tobytes() == bare["rec"].tobytes() and mist.mist_stats(gen)["slices_fetched"] == 0
    gen.shadow_map_destroy(fresh)
    _, again = mist.mist_apply(gen, cam, out, shadow, GPU_OPTS)
    assert again.tobytes() == out.tobytes() and mist.mist_stats(gen)["pixels"] == 0  # twice is once
    dead = look(**dict(GPU_CAM, width=width, height=height))
    dead.position[1] = float("nan")
    img, out = mist.mist_apply(gen, dead, rec, shadow, GPU_OPTS, rgba=True)
    assert out.tobytes() == rec.tobytes() and np.array_equal(img, _rgba8(rec["color"]))
    lib = _lib.load()
    img = np.zeros((height, width, 4), np.uint8)
    assert lib.ow_mist_apply(gen.context, shadow.handle, C.byref(cam), None, None, img.ctypes.data) == _lib.OW_ERR_INVALID and not img.any()
    other = make_gen(128, [0])[0]
    with pytest.raises(_lib.OceanWavesError) as e:
        mist.mist_apply(other, cam, rec, shadow, GPU_OPTS)                         # a map of another context
    assert e.value.status == _lib.OW_ERR_INVALID
    other.free()
    close_scene(gen, bodies, solid, shadow)


@pytest.mark.gpu
def test_gpu_async_form_in_stream_order_equals_the_host_form():
    """ow_mist_apply_async on device buffers straight after ow_shadow_map_begin / _cast and ow_environment_apply_async, with no host step
    between: the map it reads is the one cast just before it, the records the ones fogged just before it"""
    import torch
    gen, params, bodies, solid, shadow = gpu_scene()
    cam = look(**dict(GPU_CAM, width=64, height=40))
    rec = identity_records(cam, seed=9)
    env = dict(depth_begin=10.0, depth_end=90.0)
    opts = dict(GPU_OPTS, shadow_bias=0.5)
    fogged = gen.environment_apply(cam, rec, None, env)
    want_rgba, want = mist.mist_apply(gen, cam, fogged, shadow, opts, rgba=True)
    want_stats = mist.mist_stats(gen)
    assert want_stats["slices_shadowed"] > 20
    rgba_dev, rec_dev = device_buffers(cam)
    rec_dev.copy_(torch.from_numpy(np.frombuffer(rec.tobytes(), np.uint8).reshape(rec.size, -1).copy()))
    torch.cuda.synchronize()
    syncs = gen.sync_stats()
    gen.shadow_map_begin(shadow, dict(GPU_FRAME, center=(90.0, 0.0, 8.5)))        # a frame that misses the crates ...
    gen.shadow_map_cast(shadow, solid, bodies, first=0, count=3)
    gen.shadow_map_begin(shadow, GPU_FRAME)                                        # ... replaced, in stream order, by the one that holds them
    gen.shadow_map_cast(shadow, solid, bodies, first=0, count=3)
    gen.environment_apply_async(cam, rec_dev, None, env)
    mist.mist_apply_async(gen, cam, rec_dev, shadow, rgba_dev, opts)
    assert gen.sync_stats() == syncs                                               # enqueue only
    gen.sync()
    assert records_of(cam, rec_dev).tobytes() == want.tobytes()
    assert rgba_dev.cpu().numpy().reshape(cam.height, cam.width, 4).tobytes() == want_rgba.tobytes()
    assert mist.mist_stats(gen) == dict(want_stats, passes=want_stats["passes"] + 1)
    assert mist.mist_stats(gen, counters=False) == {"passes": want_stats["passes"] + 1}
    for bad in (rec_dev.data_ptr() + 4,):
        with pytest.raises(_lib.OceanWavesError):
            mist.mist_apply_async(gen, cam, bad, shadow, rgba_dev, opts)
    with pytest.raises(_lib.OceanWavesError):
        mist.mist_apply_async(gen, cam, rec_dev, shadow, rgba_dev.data_ptr() + 2, opts)
    close_scene(gen, bodies, solid, shadow)


@pytest.mark.gpu
def test_gpu_whole_frame_through_present_is_finite_and_shows_the_mist():
    """water -> solids -> ow_shadow_apply -> ow_environment_apply -> ow_mist_apply -> ow_present on the wrapper's synchronous calls: finite,
    and not the frame without the pass"""
    gen, params, bodies, solid, shadow = gpu_scene()
    sc = scales_of(params)
    gen.run(UPDATE_DELTA, params, 10)
    cam = look(**dict(GPU_CAM, width=64, height=40))
    mesh = gen.mesh_create(*grid(32, 4.0))
    _, bg = gen.mesh_draw(mesh, cam, W.clipmap_origin(cam.position, 4.0), sc)
    _, mid = gen.solid_draw(solid, bodies, cam, pixels=bg)
    _, dark = gen.shadow_apply(shadow, cam, mid, dict(receive_water=True))
    env = gen.environment_apply(cam, dark)
    _, misted = mist.mist_apply(gen, cam, env, shadow)
    with_mist, lin = gen.present(cam, misted, linear=True)
    without = gen.present(cam, env)
    assert np.isfinite(misted["color"]).all() and np.isfinite(lin).all()
    assert (misted["status"] & MIST).all() and not (env["status"] & MIST).any()
    assert with_mist.tobytes() != without.tobytes() and (with_mist[..., :3].astype(int) - without[..., :3].astype(int)).any(-1).mean() > 0.5
    assert mist.mist_stats(gen)["slices_fetched"] > 0
    gen.mesh_destroy(mesh)
    close_scene(gen, bodies, solid, shadow)


@pytest.mark.gpu
def test_the_c_example_writes_the_python_wrappers_image(tmp_path):
    """examples/mist_host.c at 256^2, a 48 x 32 PPM of 96 x 64 records, 20 steps, a 256^2 shadow map, 32 slices, against the wrapper"""
    exe = build_example(tmp_path, "mist_host")
    ppm = str(tmp_path / "mist.ppm")
    r = subprocess.run([exe, ppm, "48", "32", "20", "256", "2", "256", "32"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    kv = dict(p.split("=") for p in r.stdout.split())
    assert kv["finite"] == "1" and (kv["record_width"], kv["record_height"], kv["shadow_size"], kv["passes"], kv["pixels"]) == ("96", "64", "256", "1", str(96 * 64))
    raw = open(ppm, "rb").read()
    head = b"P6\n48 32\n255\n"
    assert raw.startswith(head) and len(raw) == len(head) + 48 * 32 * 3
    gen, params = make_gen(256, [0, 1, 2])
    sc = scales_of(params)
    bodies = gen.bodies_create(*example_crates())
    for _ in range(20):
        gen.update_all(UPDATE_DELTA, params)
        gen.bodies_step(bodies, sc, 4, UPDATE_DELTA / 4, {"warm_start": True})
    cam = W.camera((0.0, 10.0, -25.0), REF_BASIS, 75.0, 96, 64, 4000.0)
    mesh = gen.mesh_create(*grid(128, 4.0))
    _, bg = gen.mesh_draw(mesh, cam, W.clipmap_origin(cam.position, 4.0), sc, {"falloff": True, "cull_back": True})
    solid = gen.solid_create(*box(CRATE_SHAPE))
    _, mid = gen.solid_draw(solid, bodies, cam, pixels=bg)
    shadow = gen.shadow_map_create(256)
    gen.shadow_map_begin(shadow, dict(center=(0.0, 0.0, 10.0), half_extent=40.0, depth_range=80.0))
    gen.shadow_map_cast(shadow, solid, bodies)
    _, shaded = gen.shadow_apply(shadow, cam, mid, dict(receive_water=True))
    env = gen.environment_apply(cam, shaded)
    _, rec = mist.mist_apply(gen, cam, env, shadow, dict(slices=32))
    st = mist.mist_stats(gen)
    rgba = gen.present(cam, rec, {"downsample": 2})
    assert np.frombuffer(raw[len(head):], np.uint8).reshape(32, 48, 3).tobytes() == rgba[..., :3].tobytes()
    assert (int(kv["slices_fetched"]), int(kv["slices_shadowed"])) == (st["slices_fetched"], st["slices_shadowed"]) and st["slices_shadowed"] > 100
    assert int(kv["misted_pixels"]) == 96 * 64
    for h, fn in ((shadow, gen.shadow_map_destroy), (solid, gen.solid_destroy), (mesh, gen.mesh_destroy), (bodies, gen.bodies_destroy)):
        fn(h)
    gen.free()

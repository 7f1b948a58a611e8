"""The finishing stage of a camera picture (include/ocean_waves.h ow_sky_*, ow_environment_apply, ow_present): a panorama sky for the pixels
nothing was drawn into, depth or exponential fog over the others, then resolve, tonemap, transfer curve, adjustments and RGBA8
(godotoceanwaves_amd/csrc/ow_environment.h).

CPU: the ABI, the documents and the argument checks without a device; ow_environment.h compiled as plain C++
(tests/environment/environment_harness.cpp, g++ -ffp-contract=off) held to its exact cases (the fog's ends, neutral adjustments, the plain
path, constant pictures, idempotence, a 4 x 2 panorama, the seam, the sRGB round trip, the filmic curve), to atan2_f32's and acos_f32's
measured error, to an FP64 twin written from the definition (tests/environment_twin.py) on a synthetic record field and on pictures of
ow_mesh_draw's CPU build over a calm and a generated sea, and to finite outputs on awkward inputs; the stand-alone harness runs under the
sanitizers on the same inputs; the C example compiles.  GPU: the device's records, linear pixels and RGBA8 words are the CPU build's bit for
bit at sizes with partial waves and at every downsample; a whole frame (mesh draw, solids, environment, billboards, present, all
asynchronous on device buffers) equals the CPU chain, repeats to the byte and synchronises nothing; the asynchronous forms are ordered on
the context's and on a caller's stream; foreign and orphaned skies are refused; examples/present_host.c writes the wrapper's picture."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import environment_twin as ET
import helpers as H
from godotoceanwaves_amd import _lib, build
from godotoceanwaves_amd.presets import UPDATE_DELTA
from godotoceanwaves_amd.wave_generator import WaveGenerator as W
import checks as S
from checks import check_declared_and_bound, exported_symbols, HEADER, same_records
from cpu_builds import (cpu_billboard_draw, cpu_environment, cpu_mesh_draw, cpu_present, cpu_solid_draw, CSRC, ENV_CASE, env_case, ENV_DEFAULTS,
                        PRESENT_CASE, present_case, PRESENT_DEFAULTS, ROOT, sky_lookup)
from cpu_builds import billboard_harness, env_harness as harness, mesh_harness, pictures, solid_harness  # noqa: F401 (fixtures)
from scenes import (bare_context, billboards, box, camera_words, CRATE_CAM, CRATE_SHAPE, device_frame, ENV, example_crates, example_panorama,
                    example_textures, f32_options, FOAM, FRAME_CAM, FRAME_ENV, FRAME_PRESENT, frame_scene, FRAME_SHAPE, FRAME_WATER,
                    gpu_maps, gpu_material, gpu_sky, gradient_panorama, grid, HIT, level_camera, look, make_gen, material, MAX_ALPHA,
                    pose_transforms, records_of, REF_BASIS, rel, scales_of, sky_of, SOLID, SUN, synthetic_records, WHITE)
from cpu_builds import build_example, build_sanitized_harness, layout_probe

MARGINS = os.path.join(ROOT, "profiles", "present_margins.txt")
NEW_FUNCTIONS = ("ow_sky_options_default", "ow_environment_options_default", "ow_present_options_default", "ow_sky_create", "ow_sky_destroy",
                 "ow_environment_apply", "ow_environment_apply_async", "ow_present", "ow_present_async")
TOL = H.TOL_F32     # 1e-4: the project's FP32 parity tolerance
PLAIN = dict(downsample=1, tonemap=0, exposure=1.0, white=1.0, srgb=0, brightness=1.0, contrast=1.0, saturation=1.0)
ATAN2_MAX_ULP = 2.54     # measured on the CPU build over the sweep below (2.539 at y / x = -0.4148); csrc/ow_environment.h states it
ATAN2_MAX_ABS = 3.0e-7   # ... and 2.97e-7 absolute
ACOS_MAX_ABS = 3.2e-7    # ... and acos_f32's 3.12e-7 over [-1, 1], the poles included


# ---- panoramas, records and the CPU build -------------------------------------------------------------------------------------------------

def twin_environment(records, cam, opts=None, sky=None):
    o = f32_options(ENV_DEFAULTS, opts)
    if sky is None:
        return ET.environment(records, camera_words(cam), o)
    return ET.environment(records, camera_words(cam), o, sky["image"], sky["srgb"], sky["energy"])


def twin_present(records, opts=None):
    return ET.present(records, f32_options(PRESENT_DEFAULTS, opts))


def check_environment_against_twin(got, tw, records, sky, opts, what):
    """color, status and every stage the harness exposes, on every pixel; returns the margins"""
    rec = got["rec"]
    o = f32_options(ENV_DEFAULTS, opts)
    assert np.array_equal(rec["status"], tw["status"]), what
    for f in W.RENDER_PIXEL.names:
        if f not in ("color", "status"):
            assert rec[f].tobytes() == records[f].tobytes(), (what, f)
    hit = tw["hit"] & tw["todo"]
    needed = tw["todo"] & (hit & (o["aerial_perspective"] > 0) | ~tw["hit"] & (sky is not None))
    m = dict(color=rel(rec["color"], tw["color"]), ray=rel(got["ray"][tw["todo"]], tw["ray"][tw["todo"]]), sky=rel(got["sky"][needed], tw["sky"][needed]),
             amount=rel(got["amount"][hit], tw["amount"][hit]), fog=rel(got["fog"][hit], tw["fog"][hit]))
    assert max(m.values()) <= TOL, (what, m)
    assert np.isfinite(rec["color"]).all(), what
    return m


def check_present_against_twin(got, tw, what):
    """linear_out and every stage within TOL, every RGBA8 byte b within 0.5 + 255 TOL of 255 v, v the twin's unrounded value; no pixel is
    left out; returns the margins (bytes: the largest |b - 255 v| - 0.5, in byte units)"""
    m = {k: rel(got[k], tw[k]) for k in ("linear", "exposed", "mapped", "encoded", "adjusted")}
    assert max(m.values()) <= TOL, (what, m)
    b = np.abs(got["rgba"][..., :3].astype(np.float64) - 255.0 * tw["value"])
    assert (got["rgba"][..., 3] == 255).all(), what
    m["bytes"] = float(b.max()) - 0.5
    assert b.max() <= 0.5 + 255.0 * TOL, (what, m)
    return m


# ---- 1. the interface and the documents --------------------------------------------------------------------------------------------------

def test_header_declares_the_new_calls_and_the_library_exports_them():
    build.build_library()
    lib = _lib.load()
    text = check_declared_and_bound(lib, NEW_FUNCTIONS)
    exported = exported_symbols()
    assert sorted(s for s in exported if re.search(r"ow_(sky|environment|present)", s)) == sorted(NEW_FUNCTIONS)      # no group form
    assert lib.ow_abi_version() == 4 and re.search(r"#define OW_ABI_VERSION 4\b", HEADER)
    for define, value in (("OW_RAY_ENVIRONMENT", 32), ("OW_SKY_MAX_SIDE", 8192), ("OW_PRESENT_MAX_DOWNSAMPLE", 4), ("OW_FOG_EXPONENTIAL", 0),
                          ("OW_FOG_DEPTH", 1), ("OW_TONEMAP_LINEAR", 0), ("OW_TONEMAP_REINHARD", 1), ("OW_TONEMAP_FILMIC", 2)):
        assert re.search(r"#define %s %d\b" % (define, value), HEADER) and getattr(_lib, define) == value, define
    assert "No sky model, fog, tonemapping" not in HEADER
    view = HEADER.split("Camera views of the water")[1].split("#define OW_RENDER_MAX_SIDE")[0]
    assert "ow_environment_apply and ow_present" in view
    solids = HEADER.split("Solids drawn into a camera view")[1].split("#define OW_RAY_SOLID")[0]
    assert "water -> solids -> ow_environment_apply ->" in solids and "billboards -> ow_present" in solids
    section = HEADER.split("Finishing a picture: sky, fog, tonemap, sRGB")[1].split("several devices")[0]
    for cite in ("-> ow_environment_apply -> billboards (ow_billboard_draw) -> ow_present", "ow_environment.h", "UNBLURRED", "height fog, volumetric fog",
                 "FogVolume", "ACES", "not fogged", "no group form", "OW_RAY_ENVIRONMENT", "atan2_f32(0, 0) = 0", "THIS LIBRARY'S CHOICE"):
        assert cite in section, cite
    # the defaults are main.tscn:22-41 and :112-113
    e = _lib.ow_environment_options()
    lib.ow_environment_options_default(C.byref(e))
    f32 = lambda v: [float(np.float32(x)) for x in v]   # noqa: E731
    assert (e.fog_mode, e.density, e.depth_begin, e.depth_end, e.depth_curve) == (1, 1.0, 200.0, 350.0, 0.25)
    assert e.aerial_perspective == np.float32(0.626) and e.sun_scatter == np.float32(0.05) and e.flags == 0 and not any(e.reserved)
    assert list(e.light_color) == f32((0.272954, 0.419272, 0.484632)) and list(e.sun_direction) == f32(SUN) and list(e.sun_color) == [1.0, 1.0, 1.0]
    r = _lib.ow_render_options()
    lib.ow_render_options_default(C.byref(r))
    assert list(e.sky_color) == list(r.sky_color) and list(e.sun_direction) == list(r.light_direction)
    p = _lib.ow_present_options()
    lib.ow_present_options_default(C.byref(p))
    assert (p.downsample, p.tonemap, p.exposure, p.white, p.srgb, p.flags) == (1, 2, 1.0, 1.0, 1, 0) and not any(p.reserved)
    assert [p.brightness, p.contrast, p.saturation] == f32((0.85, 1.07, 1.5))
    s = _lib.ow_sky_options()
    lib.ow_sky_options_default(C.byref(s))
    assert (s.srgb, s.energy) == (1, 1.0) and not any(s.reserved)
    for fn in (lib.ow_sky_options_default, lib.ow_environment_options_default, lib.ow_present_options_default):
        fn(None)
    assert ENV_DEFAULTS["sky_color"] == tuple(round(float(v), 6) for v in r.sky_color)


def test_option_structs_agree_in_c_ctypes_and_the_harness(tmp_path, harness):
    got = {}
    for S, name in ((_lib.ow_sky_options, "ow_sky_options"), (_lib.ow_environment_options, "ow_environment_options"),
                    (_lib.ow_present_options, "ow_present_options")):
        fields = [f for f, _ in S._fields_]
        expr = ", ".join(["sizeof(%s)" % name] + ["offsetof(%s, %s)" % (name, f) for f in fields])
        src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ocean_waves.h"\nint main(void){printf("%s\\n", ' % " ".join(["%zu"] * (1 + len(fields)))
               + expr + ");return 0;}\n")
        vals = layout_probe(tmp_path, (name + "_layout"), src)
        assert vals == [C.sizeof(S)] + [getattr(S, f).offset for f in fields], name
        got[name] = dict(zip(["size"] + fields, vals))
    assert (got["ow_sky_options"]["size"], got["ow_environment_options"]["size"], got["ow_present_options"]["size"]) == (32, 128, 64)
    sizes = (C.c_int * 12)()
    harness.harness_environment_sizes(sizes)
    e, p = got["ow_environment_options"], got["ow_present_options"]
    assert list(sizes) == [32, got["ow_sky_options"]["energy"], 128, e["flags"], e["light_color"], e["sun_direction"], e["reserved"], 64, p["srgb"],
                           p["reserved"], ENV_CASE.itemsize, PRESENT_CASE.itemsize]
    assert W.RENDER_PIXEL.fields["color"][1] == 100 and W.RENDER_PIXEL.fields["status"][1] == 4 and W.RENDER_PIXEL.itemsize == 128


def test_the_documents_name_the_new_calls():
    for name in NEW_FUNCTIONS:
        assert "`%s`" % name in S.DOC.split("## 7. Index")[1], name
    for name in ("ow_sky_create", "ow_environment_apply_async", "ow_present_async"):
        assert re.search(r"\[DllImport\(Lib\)\]\s*public static extern \w+ %s\(" % name, S.SHIM), name
    for doc, words in (("README.md", ("ow_environment_apply", "ow_present")), ("DESIGN.md", ("k_environment_apply", "k_present", "128-byte")),
                       ("INTEGRATION.md", ("ow_environment_apply_async", "ow_present_async", "OW_RAY_ENVIRONMENT",
                                           "water -> solids -> ow_environment_apply -> billboards -> ow_present"))):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)
    for path in ("scripts/present_time.py", "examples/present_host.c"):
        assert os.path.exists(os.path.join(ROOT, path)), path


def test_example_builds_as_c99(tmp_path):
    build.build_library()
    build_example(tmp_path, "present_host")


# ---- 2. argument errors without a device ---------------------------------------------------------------------------------------------------

def test_argument_errors_without_a_device():
    lib = _lib.load()
    cam = level_camera(24, 12)
    rec = np.zeros((12, 24), W.RENDER_PIXEL)
    rgba = np.zeros((12, 24, 4), np.uint8)
    lin = np.zeros((12, 24, 4), np.float32)
    fake = C.c_void_p(16)   # never read: every case fails before a handle is looked at

    def env(camera, opts, rec_p=rec.ctypes.data, sky=None):
        cp, op = (C.byref(camera) if camera is not None else None), (C.byref(opts) if opts is not None else None)
        out = []
        for fn in (lib.ow_environment_apply, lib.ow_environment_apply_async):
            assert fn(None, sky, cp, op, rec_p) == _lib.OW_ERR_INVALID
            out.append(lib.ow_last_error().decode())
        assert out[0] == out[1]
        return out[0]

    def present(camera, opts, rec_p=rec.ctypes.data, rgba_p=rgba.ctypes.data, lin_p=lin.ctypes.data):
        cp, op = (C.byref(camera) if camera is not None else None), (C.byref(opts) if opts is not None else None)
        out = []
        for fn in (lib.ow_present, lib.ow_present_async):
            assert fn(None, cp, op, rec_p, rgba_p, lin_p) == _lib.OW_ERR_INVALID
            out.append(lib.ow_last_error().decode())
        assert out[0] == out[1]
        return out[0]

    eo, po = W.environment_options, W.present_options
    assert "null context" in env(cam, None) and "null context" in env(cam, None, sky=fake)     # everything else is in order
    assert "null context" in env(cam, eo(dict(fog_mode="exponential", density=0.01, depth_begin=5.0, depth_end=5.0, depth_curve=100.0, aerial_perspective=0.0)))
    assert "the records" in env(cam, None, None)
    assert "null camera" in env(None, None)
    for w, h in ((0, 12), (24, 0), (_lib.OW_RENDER_MAX_SIDE + 1, 12)):
        assert "camera size" in env(level_camera(w, h), None) and "camera size" in present(level_camera(w, h), None)
    bad = level_camera(24, 12)
    bad.reserved[1] = 7
    assert "ow_camera.reserved" in env(bad, None) and "ow_camera.reserved" in present(bad, None)
    nan, inf = float("nan"), float("inf")
    assert "fog_mode" in env(cam, eo(dict(fog_mode=2))) and "fog_mode" in env(cam, eo(dict(fog_mode=-1)))
    for key, values in (("density", (-1.0, nan, inf, 2e12)), ("depth_begin", (-1.0, nan, 400.0)), ("depth_end", (100.0, nan, inf)),
                        ("depth_curve", (0.0, 0.001, 101.0, nan)), ("aerial_perspective", (-0.1, 1.5, nan)), ("sun_scatter", (-1.0, nan, inf))):
        for v in values:
            assert key.split("_")[0] in env(cam, eo({key: v})), (key, v)
    for key in ("light_color", "sun_color", "sun_direction", "sky_color"):
        for v in (nan, inf, 3e38):
            assert "not finite" in env(cam, eo({key: (0.5, v, 0.5)})), (key, v)
    assert "zero length" in env(cam, eo(dict(sun_direction=(0.0, 0.0, 0.0))))
    o = eo({})
    o.flags = 1
    assert "environment flags" in env(cam, o)
    o = eo({})
    o.reserved[11] = 1
    assert "ow_environment_options.reserved" in env(cam, o)
    # the present
    assert "null context" in present(cam, None) and "null context" in present(cam, None, rgba_p=None) and "null context" in present(cam, None, lin_p=None)
    assert "null context" in present(cam, po(dict(downsample=4, tonemap="reinhard", white=16.0, exposure=0.0, srgb=0, brightness=8.0, contrast=0.0)))
    assert "null context" in present(cam, po(dict(downsample=0)))
    assert "both outputs" in present(cam, None, rgba_p=None, lin_p=None)
    assert "the records" in present(cam, None, rec_p=None)
    assert "null camera" in present(None, None)
    for s in (-1, 5):
        assert "downsample" in present(cam, po(dict(downsample=s)))
    assert "does not divide" in present(level_camera(25, 12), po(dict(downsample=2))) and "does not divide" in present(level_camera(24, 10), po(dict(downsample=3)))
    for t in (-1, 3):
        assert "tonemap" in present(cam, po(dict(tonemap=t)))
    for key, values in (("exposure", (-1.0, nan, 2e6)), ("white", (0.0, 0.001, nan, inf)), ("brightness", (-0.1, 9.0, nan)), ("contrast", (-0.1, 9.0)),
                        ("saturation", (nan, 8.5))):
        for v in values:
            assert ("brightness" if key in ("contrast", "saturation") else key) in present(cam, po({key: v})), (key, v)
    o = po({})
    o.srgb = 2
    assert "srgb" in present(cam, o)
    o = po({})
    o.flags = 4
    assert "present flags" in present(cam, o)
    o = po({})
    o.reserved[6] = 1
    assert "ow_present_options.reserved" in present(cam, o)
    assert not rec.tobytes().strip(b"\0") and not rgba.any() and not lin.any()
    # the sky
    img = gradient_panorama(8, 4)

    def create(opts=None, p=img.ctypes.data, w=8, h=4):
        out = C.c_void_p(0x5EED)
        assert lib.ow_sky_create(None, C.byref(opts) if opts is not None else None, p, w, h, C.byref(out)) == _lib.OW_ERR_INVALID
        assert out.value == 0x5EED
        return lib.ow_last_error().decode()

    assert "null context" in create() and "null context" in create(W.sky_options(dict(srgb=0, energy=0.0)))
    for kw in (dict(w=0), dict(h=0), dict(w=_lib.OW_SKY_MAX_SIDE + 1), dict(h=-3)):
        assert "panorama size" in create(**kw), kw
    for v in (-1.0, nan, inf, 2e12):
        assert "energy" in create(W.sky_options(dict(energy=v))), v
    o = W.sky_options({})
    o.srgb = 2
    assert "srgb" in create(o)
    o = W.sky_options({})
    o.reserved[0] = 1
    assert "ow_sky_options.reserved" in create(o)
    assert "null argument" in create(p=None)
    assert lib.ow_sky_create(None, None, img.ctypes.data, 8, 4, None) == _lib.OW_ERR_INVALID
    lib.ow_sky_destroy(None, None)
    for bad_call in (lambda: W.environment_options({"near": 1.0}), lambda: W.present_options({"gamma": 2.2}), lambda: W.sky_options({"blur": 1})):
        with pytest.raises(ValueError):
            bad_call()


# ---- 3. atan2_f32 and acos_f32 against the FP64 library -------------------------------------------------------------------------------------

def test_atan2_f32_and_acos_f32_against_the_fp64_library(harness):
    n = 1 << 20
    a = np.linspace(-np.pi, np.pi, n, endpoint=False)
    mag = 10.0 ** np.random.default_rng(7).uniform(-30, 30, n)
    ax, ay = np.float64([0, 1, 0, -1, 1, 1, -1, -1]), np.float64([1, 0, -1, 0, 1, -1, 1, -1])        # the axes and the diagonals
    tiny = 10.0 ** np.arange(-30, 1.0)
    seam_y, seam_x = np.concatenate([tiny, -tiny]), -np.ones(2 * len(tiny))                         # either side of the seam
    pole_y, pole_x = np.concatenate([tiny, tiny]), np.concatenate([np.ones(len(tiny)), -np.ones(len(tiny))])   # acos's arguments at the poles
    ys = np.concatenate([np.sin(a) * mag, ay, ay * 1e-20, seam_y, pole_y, np.sin(a)]).astype(np.float32)
    xs = np.concatenate([np.cos(a) * mag, ax, ax * 1e-20, seam_x, pole_x, np.cos(a)]).astype(np.float32)
    ys, xs = np.where(ys == 0, np.float32(0), ys), np.where(xs == 0, np.float32(0), xs)             # a zero of either sign counts as +0
    got = np.zeros(len(ys), np.float32)
    harness.harness_atan2(ys.ctypes.data, xs.ctypes.data, len(ys), got.ctypes.data)
    want = np.arctan2(ys.astype(np.float64), xs.astype(np.float64))
    assert np.isfinite(got).all() and (np.abs(got) <= np.float32(np.pi)).all()
    ulp = np.spacing(np.maximum(np.abs(want), 1.17549435e-38).astype(np.float32)).astype(np.float64)
    err, absolute = np.abs(got - want) / ulp, np.abs(got - want)
    k = err.argmax()
    print(f"atan2_f32: largest error {err.max():.3f} ulp at y / x = {ys[k] / xs[k]!r}, mean {err.mean():.3f}; {absolute.max():.3e} absolute")
    assert err.max() <= ATAN2_MAX_ULP and absolute.max() <= ATAN2_MAX_ABS
    comment = open(os.path.join(CSRC, "ow_environment.h")).read().split("OW_DEV float atan2_f32")[0]
    assert "%.2f ulp" % ATAN2_MAX_ULP in comment and "3.0e-7 absolute" in comment and "3.2e-7" in comment
    # the exact values the lookup relies on: the axes are exact quarter turns over FP32's 2 pi, and (0, 0) is 0
    two_pi, pi = np.float32(6.28318548), np.float32(3.14159274)
    exact = np.float32([[0, 0], [0, 1], [1, 0], [0, -1], [-1, 0], [-0.0, -0.0], [0, -0.0], [np.nan, 1], [1, np.inf], [np.inf, np.inf]])
    ye, xe = exact[:, 0].copy(), exact[:, 1].copy()
    out = np.zeros(len(exact), np.float32)
    harness.harness_atan2(ye.ctypes.data, xe.ctypes.data, len(exact), out.ctypes.data)
    assert list(out) == [0, 0, pi / 2, pi, -pi / 2, 0, 0, 0, 0, 0] and out[2] / two_pi == 0.25 and out[3] / two_pi == 0.5
    yy = np.concatenate([np.linspace(-1, 1, n), 1 - 10.0 ** np.arange(-8, 0.0), -1 + 10.0 ** np.arange(-8, 0.0), [1, -1, 0]]).astype(np.float32)
    g = np.zeros(len(yy), np.float32)
    harness.harness_acos(yy.ctypes.data, len(yy), g.ctypes.data)
    e = np.abs(g - np.arccos(yy.astype(np.float64)))
    print(f"acos_f32: largest error {e.max():.3e} at y = {yy[e.argmax()]!r}")
    assert e.max() <= ACOS_MAX_ABS and g[-3] == 0 and g[-2] == pi and g[-1] / pi == 0.5 and (g >= 0).all() and (g <= pi).all()
    odd = np.float32([np.nan, 2.0, -2.0, np.inf])
    g = np.zeros(4, np.float32)
    harness.harness_acos(odd.ctypes.data, 4, g.ctypes.data)
    assert np.isfinite(g).all()


# ---- 4. exact cases on the CPU build -------------------------------------------------------------------------------------------------------

def fog_amounts(L, d, opts):
    d = np.ascontiguousarray(d, np.float32)
    out = np.zeros(len(d), np.float32)
    L.harness_fog_amount(env_case(level_camera(4, 4), opts).ctypes.data, d.ctypes.data, len(d), out.ctypes.data)
    return out


def test_fog_amount_is_exact_at_and_beyond_both_ends(harness):
    f = np.float32
    below = f([0.0, 1e-30, 1.0, 199.0, np.nextafter(f(200), f(0)), 200.0])
    beyond = f([350.0, np.nextafter(f(350), f(400)), 351.0, 1000.0, 3e38])
    for density in (0.0, 0.4, 1.0, 3.0):
        for curve in (0.01, 0.25, 1.0, 100.0):
            o = dict(density=density, depth_curve=curve)
            assert (fog_amounts(harness, below, o) == 0).all(), (density, curve)
            assert (fog_amounts(harness, beyond, o) == f(min(max(density, 0.0), 1.0))).all(), (density, curve)
            inside = fog_amounts(harness, np.linspace(200, 350, 301), o)
            assert (np.diff(inside) >= 0).all() and inside[0] == 0 and inside[-1] == f(min(density, 1.0)), (density, curve)
    step = dict(depth_begin=250.0, depth_end=250.0, density=0.7)                         # a zero-size range is a step at begin
    assert list(fog_amounts(harness, f([0, 249.99, 250.0, np.nextafter(f(250), f(300)), 1e6]), step)) == [0, 0, 0, f(0.7), f(0.7)]
    e = fog_amounts(harness, f([0.0, 1.0, 100.0, 1e6, 3e38]), dict(fog_mode=0, density=0.01))
    assert e[0] == 0 and e[3] == 1 and e[4] == 1 and abs(float(e[2]) - (1 - np.exp(-1.0))) < 1e-6 and (np.diff(e) >= 0).all()
    assert (fog_amounts(harness, f([0.0, 50.0, 3e38]), dict(fog_mode=0, density=0.0)) == 0).all()
    assert np.isfinite(fog_amounts(harness, f([np.nan, np.inf, -np.inf, -5.0]), {})).all()
    assert np.isfinite(fog_amounts(harness, f([np.nan, np.inf, -np.inf, -5.0]), dict(fog_mode=0))).all()


def test_neutral_adjustments_the_plain_path_and_constant_pictures(harness, pictures):
    rec = pictures["calm"]["rec"]
    for opts in (dict(brightness=1.0, contrast=1.0, saturation=1.0), dict(PLAIN, tonemap=1), dict(PLAIN, srgb=1, exposure=2.5)):
        got = cpu_present(harness, synthetic_records(level_camera(40, 24), 3), opts)
        assert got["adjusted"].tobytes() == got["encoded"].tobytes(), opts                 # adjustments (1, 1, 1) return the input bits
    plain = cpu_present(harness, rec, PLAIN)                                                # downsample 1: the picture the draw itself packed
    assert plain["rgba"].tobytes() == pictures["calm"]["rgba"].tobytes()
    assert plain["linear"][..., :3].tobytes() == rec["color"].tobytes()
    assert np.array_equal(plain["linear"][..., 3], ((rec["status"] & HIT) != 0).astype(np.float32))
    assert cpu_present(harness, rec, dict(PLAIN, downsample=0))["rgba"].tobytes() == plain["rgba"].tobytes()
    # a constant picture: exactly the constant where 9 c and 16 c are exact (few significant bits), within an ulp for any c
    for color, exact in (((0.5, 0.8125, 3.0), True), ((0.1, 0.7, 3.3), False)):
        flat = np.zeros((24, 36), W.RENDER_PIXEL)
        flat["color"], flat["status"] = np.float32(color), HIT
        for s in (2, 3, 4):
            lin = cpu_present(harness, flat, dict(PLAIN, downsample=s))["linear"]
            assert lin.shape == (24 // s, 36 // s, 4) and (lin[..., 3] == 1).all()
            if exact:
                assert (lin[..., :3] == np.float32(color)).all(), (color, s)
            else:     # s s - 1 additions of at most half an ulp of the sum each, the product and the constant 1 / (s s): (s s) / 2 + 1 ulp
                assert (np.abs(lin[..., :3] - np.float32(color)) <= (s * s / 2 + 1) * np.spacing(np.float32(color))).all(), (color, s)
    half = np.zeros((4, 4), W.RENDER_PIXEL)                                                 # the hit share of a block
    half["status"][:2] = HIT
    assert (cpu_present(harness, half, dict(PLAIN, downsample=4))["linear"][..., 3] == 0.5).all()
    assert np.array_equal(cpu_present(harness, half, dict(PLAIN, downsample=2))["linear"][..., 3], np.float32([[1, 1], [0, 0]]))


def test_applying_twice_equals_applying_once(harness):
    cam = look((0.0, 8.0, 0.0), 20.0, -4.0, width=40, height=24)
    rec = synthetic_records(cam, 11)
    sky = sky_of(gradient_panorama())
    once = cpu_environment(harness, rec, cam, None, sky)["rec"]
    assert ((once["status"] & ENV) != 0).all() and ((once["status"] & ~ENV) == rec["status"]).all()
    assert once["color"].tobytes() != rec["color"].tobytes()
    twice = cpu_environment(harness, once, cam, None, sky)["rec"]
    assert twice.tobytes() == once.tobytes()
    other = cpu_environment(harness, once, cam, dict(fog_mode=0, density=0.5), None)["rec"]      # whatever the second pass's settings
    assert other.tobytes() == once.tobytes()
    part = rec.copy()
    part["status"][:, :20] |= ENV                                                             # a half-processed picture: only the rest moves
    got = cpu_environment(harness, part, cam, None, sky)["rec"]
    assert got[:, :20].tobytes() == part[:, :20].tobytes() and got["color"][:, 20:].tobytes() == once["color"][:, 20:].tobytes()


def test_a_4_by_2_panorama_returns_the_expected_texels(harness):
    """columns are centred on u = 1/8, 3/8, 5/8, 7/8 and rows on v = 1/4, 3/4: -Z (u = 1/2) falls between columns 1 and 2, +X (3/4) between 2
    and 3, +Z (the seam, u = 1 = 0) between 3 and 0, -X (1/4) between 0 and 1, each half and half and, on the horizon, half of either row; straight
    up is row 0 alone (v clamps), straight down row 1, at u = 1/2"""
    img = np.zeros((2, 4, 4), np.uint8)
    img[..., 0] = [[10, 40, 90, 160], [20, 60, 120, 250]]
    img[..., 1] = [[200, 150, 100, 50], [180, 130, 80, 30]]
    img[..., 2] = 255 - img[..., 0]
    img[..., 3] = 7                                                                # alpha is not read
    t = img[..., :3].astype(np.float64) / 255.0
    dirs = {"+X": (1, 0, 0), "-X": (-1, 0, 0), "+Z": (0, 0, 1), "-Z": (0, 0, -1), "up": (0, 1, 0), "down": (0, -1, 0)}
    cols = {"+X": (2, 3), "-X": (0, 1), "+Z": (3, 0), "-Z": (1, 2), "up": (1, 2), "down": (1, 2)}
    rows = {"up": (0,), "down": (1,)}
    got = sky_lookup(harness, sky_of(img, srgb=0), list(dirs.values()))
    for k, name in enumerate(dirs):
        want = np.mean([t[r, c] for r in rows.get(name, (0, 1)) for c in cols[name]], axis=0)
        assert np.abs(got[k] - want).max() < 2e-7, (name, got[k], want)
    lin = sky_lookup(harness, sky_of(img, srgb=1, energy=2.0), list(dirs.values()))     # through the sRGB table, times the energy
    table = ET.srgb_table()
    for k, name in enumerate(dirs):
        want = 2.0 * np.mean([table[img[r, c, :3]] for r in rows.get(name, (0, 1)) for c in cols[name]], axis=0)
        assert np.abs(lin[k] - want).max() < 1e-6, name
    assert np.abs(got - ET.sky(img, np.float64(list(dirs.values())), 0)).max() < 2e-7    # the twin reads the same texels
    one = sky_lookup(harness, sky_of(img[:1, :1], srgb=0), list(dirs.values()) + [(0.6, 0.0, 0.8)])   # a 1 x 1 panorama is one colour everywhere
    assert np.abs(one - img[0, 0, :3] / 255.0).max() < 2e-7


def test_the_two_sides_of_the_seam_blend_the_last_column_and_the_first(harness):
    w = 8
    img = np.zeros((2, w, 4), np.uint8)
    img[:, 1:w - 1, 2] = 255                      # every inner column is blue
    img[:, w - 1, 0] = 255                        # the last is red
    img[:, 0, 1] = 255                            # the first is green
    eps = np.float64([1e-7, 1e-4, 1e-2, 3e-2])
    left = np.stack([eps, np.zeros(4), np.ones(4)], axis=1)       # d.x > 0: u just below 1
    right = left * [-1, 1, 1]                                      # d.x < 0: u just above 0
    d = np.concatenate([left, right])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    got = sky_lookup(harness, sky_of(img, srgb=0), d)
    assert (got[:, 2] == 0).all() and np.abs(got[:, 0] + got[:, 1] - 1).max() < 1e-6            # red and green only, and all of it
    assert (got[:4, 0] >= 0.5).all() and (got[4:, 1] >= 0.5).all() and (np.diff(got[:4, 0]) >= 0).all() and (np.diff(got[4:, 1]) >= 0).all()
    assert abs(float(got[0, 0]) - 0.5) < 1e-6 and abs(float(got[4, 1]) - 0.5) < 1e-6            # continuous across the seam
    assert np.abs(got - ET.sky(img, d, 0)).max() < 1e-5
    on = sky_lookup(harness, sky_of(img, srgb=0), [(0.0, 0.0, 1.0), (-0.0, 0.0, 1.0)])
    assert (on == np.float32([0.5, 0.5, 0.0])).all()


def test_srgb_round_trip_of_all_256_bytes(harness):
    table = ET.srgb_table().astype(np.float32)                       # spray_srgb_table: FP64, narrowed once
    rec = np.zeros((1, 256), W.RENDER_PIXEL)
    rec["color"][0] = table[:, None]
    got = cpu_present(harness, rec, dict(PLAIN, srgb=1))
    assert np.array_equal(got["rgba"][0, :, :3], np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)) and (got["rgba"][..., 3] == 255).all()
    assert np.abs(got["encoded"][0, :, 0].astype(np.float64) - np.arange(256) / 255.0).max() < 2e-6
    assert cpu_present(harness, rec, PLAIN)["rgba"][0, 128, 0] == 55                  # without the curve a viewer gets the dark, linear bytes


def test_the_filmic_curve(harness):
    for white in (1.0, 4.0, 16.0):
        c = np.unique(np.concatenate([np.linspace(0.0, 16.0, 4097), np.geomspace(1e-3, 50.0, 512), [white]]).astype(np.float32))
        rec = np.zeros((1, len(c)), W.RENDER_PIXEL)
        rec["color"][0] = c[:, None]
        got = cpu_present(harness, rec, dict(PLAIN, tonemap=2, white=white))["mapped"][0, :, 0]
        assert got[0] == 0 and (np.diff(got) >= 0).all(), white                       # filmic of 0 is exactly 0; monotone
        assert abs(float(got[c == np.float32(white)][0]) - 1.0) <= TOL, white         # filmic at white is 1
        assert rel(got, ET.tonemap(c.astype(np.float64), 2, white)) <= TOL
        r = cpu_present(harness, rec, dict(PLAIN, tonemap=1, white=white))["mapped"][0, :, 0]
        assert r[0] == 0 and (np.diff(r) >= 0).all() and abs(float(r[c == np.float32(white)][0]) - 1.0) <= TOL and rel(r, ET.tonemap(c.astype(np.float64), 1, white)) <= TOL


# ---- 5. against the FP64 twin --------------------------------------------------------------------------------------------------------------

ENV_VARIANTS = {"the scene's": None, "exponential": dict(fog_mode=0, density=0.004, aerial_perspective=0.0, sun_scatter=0.0),
                "thin, curved, bright sun": dict(density=0.6, depth_curve=2.0, depth_begin=50.0, depth_end=900.0, sun_scatter=0.8, sun_color=(3.0, 2.5, 2.0),
                                                 aerial_perspective=1.0)}
PRESENT_VARIANTS = {"the scene's": None, "reinhard x2": dict(tonemap=1, white=4.0, exposure=1.7, downsample=2),
                    "linear x3": dict(tonemap=0, srgb=0, brightness=1.0, contrast=1.0, saturation=1.0, downsample=3),
                    "filmic x4": dict(tonemap=2, white=6.0, exposure=0.6, saturation=0.0, downsample=4)}


def test_the_pictures_meet_the_twins_conditions(pictures):
    """what the comparison below is worth: both pictures hold sky and water, the water spans the fog's whole range"""
    for name in ("calm", "sea"):
        rec = pictures[name]["rec"]
        hit = (rec["status"] & HIT) != 0
        assert 0.2 < hit.mean() < 0.8 and rec["t"][hit].min() < 100.0 and rec["t"][hit].max() > 350.0, name
        assert ((rec["t"] > 200.0) & (rec["t"] < 350.0) & hit).sum() > 20, name


def test_environment_and_present_against_the_fp64_twin(harness, pictures):
    """color, linear_out and every stage within TOL = 1e-4 relative to max(1, |value|), every byte within 0.5 + 255 TOL of the twin's unrounded
    value, on every pixel.  Measured on the CPU build (profiles/present_margins.txt, written with PRESENT_WRITE_MARGINS=1): the largest
    stage difference is 1.5e-6 (color, on the synthetic field's colours of up to 50), the others are below 1.1e-6 (fog) and 4.5e-7 (the
    present's stages); no byte is further than 0.5 from the twin's unrounded value (the largest excess is -1.1e-5 against the 2.55e-2
    allowed)."""
    cam = pictures["cam"]
    fields = {"synthetic": synthetic_records(cam, 1), "calm": pictures["calm"]["rec"], "sea": pictures["sea"]["rec"]}
    skies = {"no sky": None, "panorama": sky_of(gradient_panorama(), 1, 1.3), "raw 5 x 3": sky_of(gradient_panorama(5, 3, 9), 0, 0.5)}
    lines, worst_env, worst_present = [], {}, {}
    for fname, rec in fields.items():
        for sname, sky in skies.items():
            for ename, eopts in ENV_VARIANTS.items():
                got = cpu_environment(harness, rec, cam, eopts, sky)
                tw = twin_environment(rec, cam, eopts, sky)
                m = check_environment_against_twin(got, tw, rec, sky, eopts, (fname, sname, ename))
                lines.append("environment  %-9s %-9s %-25s " % (fname, sname, ename) + " ".join("%s %.2e" % kv for kv in m.items()))
                for k, v in m.items():
                    worst_env[k] = max(worst_env.get(k, 0.0), v)
                if sname == "raw 5 x 3":
                    continue
                for pname, popts in PRESENT_VARIANTS.items():
                    p = cpu_present(harness, got["rec"], popts)
                    pm = check_present_against_twin(p, twin_present(got["rec"], popts), (fname, sname, ename, pname))
                    lines.append("present      %-9s %-9s %-25s %-12s " % (fname, sname, ename, pname) + " ".join("%s %.2e" % kv for kv in pm.items()))
                    for k, v in pm.items():
                        worst_present[k] = max(worst_present.get(k, -1.0), v)
    print("worst environment", worst_env, "worst present", worst_present)
    if os.environ.get("PRESENT_WRITE_MARGINS") == "1":
        with open(MARGINS, "w") as f:
            f.write("ow_environment_apply and ow_present, CPU build against the FP64 twin (tests/test_environment.py): |difference| / max(1, |value|) per stage,\n"
                    "bytes = the largest |b - 255 v| - 0.5 in byte units (allowed: 255 TOL = 2.55e-2); TOL = 1e-4; 72 x 36 records, every pixel\n")
            f.write("worst environment " + " ".join("%s %.2e" % kv for kv in worst_env.items()) + "\n")
            f.write("worst present     " + " ".join("%s %.2e" % kv for kv in worst_present.items()) + "\n")
            f.write("\n".join(lines) + "\n")
    assert os.path.exists(MARGINS)


def test_billboards_blend_over_the_finished_sky_and_the_fogged_water(harness, billboard_harness, pictures):
    """the order the frame defines, on the CPU builds: ow_billboard_draw over records the pass has finished keeps status (OW_RAY_ENVIRONMENT
    included), blends dst (1 - ALPHA) + ALBEDO ALPHA over the panorama's colour where nothing was hit and over the fogged colour where water
    was, and the spray itself is never fogged: a second pass afterwards changes nothing, while fogging after the spray would"""
    cam, rec = pictures["cam"], pictures["calm"]["rec"]
    sky = sky_of(gradient_panorama(), 1, 1.3)
    passed = cpu_environment(harness, rec, cam, None, sky)
    env = passed["rec"]
    yaw, eye = np.radians(15.0), np.float64([0.0, 20.0, 0.0])

    def at(distance, elevation_deg):
        e = np.radians(elevation_deg)
        return tuple(eye + distance * np.float64([np.sin(yaw) * np.cos(e), np.sin(e), np.cos(yaw) * np.cos(e)]))

    # one billboard high over the horizon, one 150 m out and 4 degrees down: the water behind it is 200 m to 350 m away, inside the fog's range
    inst = billboards([(at(150.0, 12.0), 40.0, 20.0, 1.0, 1.0), (at(150.0, -4.0), 80.0, 10.0, 1.0, 1.0)])
    mat = material(**WHITE)
    fin = cpu_billboard_draw(billboard_harness, inst, cam, mat, time=0.5, records=env)["rec"]
    assert fin["status"].tobytes() == env["status"].tobytes() and ((fin["status"] & ENV) != 0).all()
    over_sky, over_fog = spray_over_both(fin, passed["amount"])
    assert over_sky.sum() > 20 and over_fog.sum() > 20 and (passed["amount"][over_fog] > 0.1).any()
    dry = fin["reserved"][..., 1] == 0
    assert fin["color"][dry].tobytes() == env["color"][dry].tobytes()
    albedo = np.float64(np.float32(FOAM) * np.float32((1.65, 1.75, 1.65)))
    for mask in (over_sky, over_fog):                                    # one layer each: the blend's ALPHA is the same in every channel
        one = mask & (fin["reserved"][..., 1] == 1)
        dst, out = env["color"][one].astype(np.float64), fin["color"][one].astype(np.float64)
        alpha = (out - dst) / (albedo - dst)
        assert one.sum() > 20 and (alpha > 0).all() and (alpha <= MAX_ALPHA + 1e-6).all() and np.abs(alpha - alpha[:, :1]).max() < 1e-4
    again = cpu_environment(harness, fin, cam, None, sky)["rec"]             # the spray is not fogged
    assert again.tobytes() == fin.tobytes()
    early = cpu_billboard_draw(billboard_harness, inst, cam, mat, time=0.5, records=rec)["rec"]      # the other order would fog it
    late = cpu_environment(harness, early, cam, None, sky)["rec"]
    assert np.abs(late["color"][over_fog] - fin["color"][over_fog]).max() > 1e-3
    assert cpu_present(harness, fin)["rgba"].tobytes() != cpu_present(harness, env)["rgba"].tobytes()


# ---- 6. awkward inputs ----------------------------------------------------------------------------------------------------------------------

def awkward_records(cam):
    rec = synthetic_records(cam, 21)
    flat = rec.reshape(-1)
    f = np.float32
    odd_t = f([0.0, 3e38, np.nan, np.inf, -1.0, 1e-45])
    odd_c = [(1e30, -1e30, 1e30), (np.nan, 0.5, 0.5), (np.inf, -np.inf, 0.0), (3e38, 3e38, 3e38), (-3e38, 0.0, 3e38), (-0.0, 1e-45, 50.0)]
    for k in range(len(flat)):
        if k % 3 == 0:
            flat["t"][k] = odd_t[(k // 3) % len(odd_t)]
        if k % 2 == 0:
            flat["color"][k] = f(odd_c[(k // 2) % len(odd_c)])
    return rec


def awkward_cases():
    cam = look((0.0, 8.0, 0.0), 20.0, -4.0, width=24, height=12)
    pano = gradient_panorama(16, 8)
    nan_cam = look((0.0, 8.0, 0.0), 20.0, -4.0, width=24, height=12)
    nan_cam.position[1] = float("nan")
    inf_cam = look((0.0, 8.0, 0.0), 20.0, -4.0, width=24, height=12)
    inf_cam.basis[4] = float("inf")
    flat_cam = W.camera((0, 0, 0), np.zeros((3, 3)), 75.0, 24, 12, 100.0)                    # finite, but no ray has a direction
    return {
        "odd records, the scene's": dict(cam=cam, sky=sky_of(pano)),
        "odd records, no sky": dict(cam=cam, sky=None),
        "zero-size range": dict(cam=cam, sky=sky_of(pano), env=dict(depth_begin=300.0, depth_end=300.0)),
        "curve at its lower bound": dict(cam=cam, sky=sky_of(pano), env=dict(depth_curve=0.01)),
        "curve at its upper bound": dict(cam=cam, sky=None, env=dict(depth_curve=100.0, density=1e12)),
        "exponential, huge density": dict(cam=cam, sky=sky_of(pano), env=dict(fog_mode=0, density=1e12)),
        "energy 0": dict(cam=cam, sky=sky_of(pano, 1, 0.0)),
        "a 1 x 1 panorama": dict(cam=cam, sky=sky_of(pano[:1, :1], 0, 1e12)),
        "huge colours": dict(cam=cam, sky=None, env=dict(light_color=(1e12, -1e12, 1e12), sky_color=(-1e12, 1e12, 0.0), sun_color=(1e12, 1e12, 1e12),
                                                        sun_scatter=1e12, aerial_perspective=1.0)),
        "a camera that is not a number": dict(cam=nan_cam, sky=sky_of(pano), untouched=True),
        "an infinite basis": dict(cam=inf_cam, sky=sky_of(pano), untouched=True),
        "a basis of zeros": dict(cam=flat_cam, sky=sky_of(pano)),
    }


AWKWARD_PRESENTS = (None, dict(tonemap=1, white=0.01, exposure=1e6, downsample=2), dict(tonemap=0, srgb=0, exposure=1e6, brightness=8.0, contrast=8.0,
                                                                                      saturation=8.0, downsample=3),
                    dict(tonemap=2, white=1e6, exposure=0.0, downsample=4), dict(tonemap=2, white=0.01, exposure=1e6, srgb=1, saturation=0.0))


def test_awkward_inputs_give_finite_outputs(harness):
    for name, c in awkward_cases().items():
        rec = awkward_records(c["cam"])
        got = cpu_environment(harness, rec, c["cam"], c.get("env"), c["sky"])
        out = got["rec"]
        if c.get("untouched"):
            assert out.tobytes() == rec.tobytes(), name                                  # ow_mesh_draw's rule: nothing moves, no bit is set
        else:
            assert ((out["status"] & ENV) != 0).all(), name
            hit = (rec["status"] & HIT) != 0
            written = hit | (c["sky"] is not None)                                       # a miss without a sky keeps its colour, whatever it was
            assert np.isfinite(out["color"][written]).all(), name
            assert out["color"][~written].tobytes() == rec["color"][~written].tobytes(), name
            for k in ("ray", "sky", "amount", "fog"):
                assert np.isfinite(got[k]).all(), (name, k)
            assert (got["amount"] >= 0).all() and (got["amount"] <= 1).all(), name
        for popts in AWKWARD_PRESENTS:
            p = cpu_present(harness, out, popts)
            for k in ("linear", "mapped", "encoded", "adjusted"):      # (exposed is the resolved colour times exposure: the tonemap caps it)
                assert np.isfinite(p[k]).all(), (name, popts, k)
            assert (p["rgba"][..., 3] == 255).all()


# ---- 7. the stand-alone program under the sanitizers ---------------------------------------------------------------------------------------

def write_case(path, cam, rec, env, sky, popts):
    with open(path, "wb") as f:
        f.write(env_case(cam, env, sky).tobytes())
        f.write(present_case(cam.width, cam.height, popts).tobytes())
        if sky is not None:
            f.write(sky["image"].tobytes())
        f.write(np.ascontiguousarray(rec, W.RENDER_PIXEL).tobytes())


def test_stand_alone_harness_runs_clean_under_the_sanitizers(tmp_path, harness, pictures):
    """the harness as a program of its own (-DENVIRONMENT_HARNESS_MAIN), built with -fsanitize=address,undefined, on the twin's fields and every
    awkward case: what it writes is the shared library's"""
    exe = build_sanitized_harness("environment", tmp_path)
    cam = pictures["cam"]
    cases = [("synthetic", cam, synthetic_records(cam, 1), None, sky_of(gradient_panorama(), 1, 1.3), None),
             ("sea, exponential", cam, pictures["sea"]["rec"], ENV_VARIANTS["exponential"], None, PRESENT_VARIANTS["linear x3"]),
             ("calm, raw sky", cam, pictures["calm"]["rec"], ENV_VARIANTS["thin, curved, bright sun"], sky_of(gradient_panorama(5, 3, 9), 0, 0.5),
              PRESENT_VARIANTS["filmic x4"])]
    for k, (name, c) in enumerate(awkward_cases().items()):
        cases.append((name, c["cam"], awkward_records(c["cam"]), c.get("env"), c["sky"], AWKWARD_PRESENTS[k % len(AWKWARD_PRESENTS)]))
    for k, (name, cam, rec, env, sky, popts) in enumerate(cases):
        path, out = str(tmp_path / f"case{k}.bin"), str(tmp_path / f"case{k}.out")
        write_case(path, cam, rec, env, sky, popts)
        r = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (name, r.stdout + r.stderr)
        assert r.stdout.endswith("ok\n") and "not_finite=0" in r.stdout and "idempotent=1" in r.stdout, (name, r.stdout)
        assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (name, r.stderr)
        once = cpu_environment(harness, rec, cam, env, sky)["rec"]
        p = cpu_present(harness, once, popts)
        assert open(out, "rb").read() == once.tobytes() + p["rgba"].tobytes() + p["linear"].tobytes(), name


# ---- 8-12. on the GPU -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("width,height,s", [(67, 35, 1), (69, 39, 3), (2, 2, 2)])
def test_gpu_pass_and_present_are_the_cpu_builds_bit_for_bit(harness, width, height, s):
    """67 x 35 records: partial blocks and waves on both axes; 69 x 39 at s = 3: an output of 23 x 13; 2 x 2 at s = 2: one output pixel; with and
    without a sky, depth and exponential fog, the three tonemaps; then the awkward records"""
    gen = bare_context()
    cam = look((0.0, 8.0, 0.0), 20.0, -4.0, width=width, height=height)
    rec = synthetic_records(cam, 100 + width)
    pano = sky_of(gradient_panorama(), 1, 1.3)
    handle = gpu_sky(gen, pano)
    for sky, sky_handle in ((None, None), (pano, handle)):
        for eopts in (None, ENV_VARIANTS["exponential"]):
            want = cpu_environment(harness, rec, cam, eopts, sky)["rec"]
            got = gen.environment_apply(cam, rec, sky_handle, eopts)
            same_records(got, want, (sky is not None, eopts))
            for tonemap in (0, 1, 2):
                popts = dict(tonemap=tonemap, white=3.0, exposure=1.4, downsample=s)
                p = cpu_present(harness, want, popts)
                rgba, lin = gen.present(cam, got, popts, linear=True)
                assert rgba.shape == (height // s, width // s, 4) and rgba.tobytes() == p["rgba"].tobytes(), (sky is not None, eopts, tonemap)
                assert lin.tobytes() == p["linear"].tobytes(), (sky is not None, eopts, tonemap)
            assert gen.present(cam, got, dict(PLAIN, downsample=s)).tobytes() == cpu_present(harness, want, dict(PLAIN, downsample=s))["rgba"].tobytes()
    odd = awkward_records(cam)
    want = cpu_environment(harness, odd, cam, None, pano)["rec"]
    got = gen.environment_apply(cam, odd, handle)
    same_records(got, want, "awkward")
    for popts in AWKWARD_PRESENTS:
        popts = dict(popts or {}, downsample=s)
        p = cpu_present(harness, want, popts)
        rgba, lin = gen.present(cam, got, popts, linear=True)
        assert rgba.tobytes() == p["rgba"].tobytes() and lin.tobytes() == p["linear"].tobytes() and np.isfinite(lin).all(), popts
    nan_cam = look((0.0, 8.0, 0.0), 20.0, -4.0, width=width, height=height)
    nan_cam.basis[0] = float("nan")
    assert gen.environment_apply(nan_cam, rec, handle).tobytes() == rec.tobytes()
    gen.sky_destroy(handle)
    gen.free()


                                 # spray in front of that edge lies over water and the spray behind it over pixels without a hit -- the sky


def spray_over_both(fin, amount):
    """the pixels of a finished frame that received spray: those over the sky, and those over water the pass fogged"""
    sprayed = fin["reserved"][..., 1] > 0
    hit = (fin["status"] & HIT) != 0
    return sprayed & ~hit, sprayed & hit & ((fin["status"] & SOLID) == 0) & (amount > 0)


@pytest.mark.gpu
def test_gpu_whole_frame_is_the_cpu_chain_bit_for_bit(harness, mesh_harness, solid_harness, billboard_harness):
    """256^2 x 3 cascades, 64 x 40 records: ow_mesh_draw_async -> ow_solid_draw_async on a stepped body set -> ow_environment_apply_async ->
    ow_billboard_draw_async -> ow_present_async (s = 2) on device buffers, one read-back, against the CPU builds chained in the same order;
    the frame again gives the same bytes; no call synchronised"""
    import torch
    gen, params, sc, bodies, spray = frame_scene()
    cam = look(**FRAME_CAM)
    mat = material()
    m = gpu_material(gen, mat)
    water = grid(*FRAME_WATER)
    mesh = gen.mesh_create(*water)
    shape = box(FRAME_SHAPE)
    solid = gen.solid_create(*shape)
    pano = sky_of(gradient_panorama(), 1, 1.2)
    sky = gpu_sky(gen, pano)
    origin = W.clipmap_origin(cam.position, 4.0)
    frames = [device_frame(cam, 2), device_frame(cam, 2)]
    gen.mesh_draw(mesh, cam, origin, sc)                       # the draws' scratch exists from here on
    gen.solid_draw(solid, bodies, cam, pixels=True)
    gen.spray_draw(spray, m, cam, pixels=True)
    torch.cuda.synchronize()
    syncs = gen.sync_stats()
    for rec_dev, rgba_dev, lin_dev in frames:
        gen.mesh_draw_async(mesh, cam, origin, sc, None, rec_dev)
        gen.solid_draw_async(solid, bodies, cam, None, rec_dev)
        gen.environment_apply_async(cam, rec_dev, sky, FRAME_ENV)
        gen.spray_draw_async(spray, m, cam, None, rec_dev)
        gen.present_async(cam, rec_dev, rgba_dev, lin_dev, FRAME_PRESENT)
    assert gen.sync_stats() == syncs                           # host_syncs has not moved
    gen.sync()
    got = [(records_of(cam, r), a.cpu().numpy(), l.cpu().numpy()) for r, a, l in frames]
    for a, b in zip(got[0], got[1]):
        assert a.tobytes() == b.tobytes()                      # the frame repeats to the byte
    d, nm = gpu_maps(gen, 3)
    bg = cpu_mesh_draw(mesh_harness, d, nm, sc, water, origin, cam)["rec"]
    mid = cpu_solid_draw(solid_harness, shape, pose_transforms(gen, bodies), cam, None, bg, stride=24, flags=np.zeros(8, np.int32))["rec"]
    passed = cpu_environment(harness, mid, cam, FRAME_ENV, pano)
    env = passed["rec"]
    inst, _, draw = gen.spray_read(spray)
    time = float(np.float32(gen.spray_stats(spray)["time"]))
    fin = cpu_billboard_draw(billboard_harness, inst, cam, mat, time=time, order=draw, records=env)["rec"]
    want = cpu_present(harness, fin, FRAME_PRESENT)
    rec, rgba, lin = got[0]
    same_records(rec, fin, "mesh, solids, environment, billboards")
    assert rgba.tobytes() == want["rgba"].tobytes() and lin.tobytes() == want["linear"].tobytes()
    hit = (fin["status"] & HIT) != 0
    over_sky, over_fog = spray_over_both(fin, passed["amount"])
    print(f"sky pixels {int((~hit).sum())} crate pixels {int(((fin['status'] & SOLID) != 0).sum())} fogged {int((passed['amount'] > 0).sum())} "
          f"live {len(draw)} sprayed over the sky {int(over_sky.sum())} over fogged water {int(over_fog.sum())}")
    assert ((fin["status"] & ENV) != 0).all() and (~hit).sum() > 100 and ((fin["status"] & SOLID) != 0).sum() > 20 and (passed["amount"] > 0).sum() > 100
    # the billboard stage is no bystander: spray lies over the finished sky and over fogged water, blended over the pass's colours there
    assert over_sky.sum() > 5 and over_fog.sum() > 5
    both, dry = over_sky | over_fog, ~(fin["reserved"][..., 1] > 0)
    assert (fin["color"][both] != env["color"][both]).any(axis=-1).mean() > 0.9 and fin["color"][dry].tobytes() == env["color"][dry].tobytes()
    assert want["rgba"].tobytes() != cpu_present(harness, env, FRAME_PRESENT)["rgba"].tobytes()      # ... and it reaches the presented bytes
    for h, fn in ((sky, gen.sky_destroy), (solid, gen.solid_destroy), (m, gen.spray_material_destroy), (mesh, gen.mesh_destroy), (spray, gen.spray_destroy),
                  (bodies, gen.bodies_destroy)):
        fn(h)
    gen.free()


def _order_case(stream=None, torch_stream=None):
    """ticks, then the mesh draw, the pass and the present with no host synchronisation, then more ticks, against a context that stopped after
    the first half and ran the synchronous forms: the frame saw the maps of exactly its point of the stream"""
    import torch
    a, pa = make_gen(128, [0, 1], stream=stream)
    b, pb = make_gen(128, [0, 1])
    sc = scales_of(pa)
    cam = look(**dict(CRATE_CAM, width=48, height=32))
    water = grid(32, 4.0)
    ha, hb = a.mesh_create(*water), b.mesh_create(*water)
    pano = sky_of(gradient_panorama(), 1, 1.0)
    sa, sb = gpu_sky(a, pano), gpu_sky(b, pano)
    origin = W.clipmap_origin(cam.position, 4.0)
    rec_dev, rgba_dev, lin_dev = device_frame(cam, 2)
    a.mesh_draw(ha, cam, origin, sc)                           # the mesh draw's visibility scratch exists from here on
    for g, p in ((a, pa), (b, pb)):
        g.run(UPDATE_DELTA, p, 12)
    torch.cuda.synchronize()
    syncs = a.sync_stats()

    def frame():
        a.mesh_draw_async(ha, cam, origin, sc, None, rec_dev)
        a.environment_apply_async(cam, rec_dev, sa, FRAME_ENV)
        a.present_async(cam, rec_dev, rgba_dev, lin_dev, FRAME_PRESENT)

    if torch_stream is not None:
        with torch.cuda.stream(torch_stream):
            frame()
            copy = rgba_dev.to("cpu", non_blocking=False)       # the caller's own work, ordered by its stream alone
    else:
        frame()
    for _ in range(8):
        a.update_all(UPDATE_DELTA, pa)
    assert a.sync_stats() == syncs
    a.sync()
    _, bg = b.mesh_draw(hb, cam, origin, sc)
    env = b.environment_apply(cam, bg, sb, FRAME_ENV)
    want_rgba, want_lin = b.present(cam, env, FRAME_PRESENT, linear=True)
    same_records(records_of(cam, rec_dev), env, "ordered")
    assert rgba_dev.cpu().numpy().tobytes() == want_rgba.tobytes() and lin_dev.cpu().numpy().tobytes() == want_lin.tobytes()
    if torch_stream is not None:
        assert copy.numpy().tobytes() == want_rgba.tobytes()
    later = a.present(cam, a.environment_apply(cam, a.mesh_draw(ha, cam, origin, sc)[1], sa, FRAME_ENV), FRAME_PRESENT)
    assert later.tobytes() != want_rgba.tobytes()               # the second half moved the maps
    for g, s, h in ((a, sa, ha), (b, sb, hb)):
        g.sky_destroy(s)
        g.mesh_destroy(h)
        g.free()


@pytest.mark.gpu
def test_async_forms_are_ordered_behind_a_tick_on_the_contexts_stream():
    _order_case()


@pytest.mark.gpu
def test_async_forms_are_ordered_behind_a_tick_on_a_callers_stream():
    import torch
    s = torch.cuda.Stream()
    _order_case(stream=s.cuda_stream, torch_stream=s)


@pytest.mark.gpu
def test_skies_of_other_contexts_and_orphans_are_refused_and_errors_write_nothing(harness):
    """the asynchronous forms hold no scratch: they never synchronise, whatever the size; the synchronous forms' pixel blocks grow once and are
    reused; refusals write nothing; a sky of another context is
    OW_ERR_INVALID, an orphaned one OW_ERR_STATE and still the caller's to destroy"""
    import torch
    gen, other = bare_context(), bare_context()
    pano = sky_of(gradient_panorama(), 1, 1.0)
    sky, foreign = gpu_sky(gen, pano), gpu_sky(other, pano)
    torch.cuda.synchronize()
    syncs = gen.sync_stats()
    for w, h in ((24, 12), (96, 60), (24, 12)):
        cam = level_camera(w, h)
        rec_dev, rgba_dev, lin_dev = device_frame(cam, 1)
        rec = synthetic_records(cam, w)
        rec_dev.copy_(torch.from_numpy(np.frombuffer(rec.tobytes(), np.uint8).reshape(-1, 128).copy()))
        gen.environment_apply_async(cam, rec_dev, sky)
        gen.present_async(cam, rec_dev, rgba_dev, lin_dev)
        assert gen.sync_stats() == syncs
        torch.cuda.synchronize()
        want = cpu_environment(harness, rec, cam, None, pano)["rec"]
        same_records(records_of(cam, rec_dev), want, (w, h))
        assert rgba_dev.cpu().numpy().tobytes() == cpu_present(harness, want)["rgba"].tobytes()
    # The synchronous forms have scratch: the context's two pixel blocks (the records; 20 bytes per output pixel for both outputs), grow-only and
    # shared with every synchronous picture call, with no counter of their own.  Small, large, small again: they grow once and are reused.
    for w, h, s in ((24, 12, 1), (96, 60, 2), (24, 12, 3), (96, 60, 1)):
        cam = level_camera(w, h)
        rec = synthetic_records(cam, w + s)
        want = cpu_environment(harness, rec, cam, None, pano)["rec"]
        got = gen.environment_apply(cam, rec, sky)
        same_records(got, want, (w, h, s))
        p = cpu_present(harness, want, {"downsample": s})
        rgba, lin = gen.present(cam, got, {"downsample": s}, linear=True)
        assert rgba.tobytes() == p["rgba"].tobytes() and lin.tobytes() == p["linear"].tobytes(), (w, h, s)
        assert gen.present(cam, got, {"downsample": s}).tobytes() == p["rgba"].tobytes()
    cam = level_camera(24, 12)
    rec_dev, rgba_dev, lin_dev = device_frame(cam, 1)

    def refused(fn, *args, status=_lib.OW_ERR_INVALID, **kw):
        with pytest.raises(_lib.OceanWavesError) as e:
            fn(*args, **kw)
        assert e.value.status == status

    refused(gen.environment_apply_async, cam, rec_dev, foreign)                              # another context's sky
    refused(gen.environment_apply, cam, np.zeros((12, 24), W.RENDER_PIXEL), foreign)
    refused(gen.environment_apply_async, cam, rec_dev, sky, {"density": -1.0})
    refused(gen.environment_apply_async, cam, rec_dev.data_ptr() + 4, sky)                   # records are read and written as 16-byte vectors
    refused(gen.environment_apply_async, level_camera(0, 12), rec_dev, sky)
    refused(gen.present_async, cam, rec_dev, rgba_dev, lin_dev, {"downsample": 5})
    refused(gen.present_async, level_camera(23, 12), rec_dev, rgba_dev, lin_dev, {"downsample": 2})
    refused(gen.present_async, cam, rec_dev, None, None)
    refused(gen.present_async, cam, rec_dev, rgba_dev.data_ptr() + 2, lin_dev)
    refused(gen.present_async, cam, rec_dev, rgba_dev, lin_dev.data_ptr() + 4)
    torch.cuda.synchronize()
    assert not rec_dev.any() and not rgba_dev.any() and not lin_dev.any()
    # lifetimes: the contexts go first; an orphaned sky can be destroyed and is refused by everything else
    live = bare_context()
    gen.free()
    other.free()
    lib = _lib.load()
    assert lib.ow_environment_apply_async(live.context, sky.handle, C.byref(cam), None, rec_dev.data_ptr()) == _lib.OW_ERR_STATE
    host = np.zeros((12, 24), W.RENDER_PIXEL)
    assert lib.ow_environment_apply(live.context, foreign.handle, C.byref(cam), None, host.ctypes.data) == _lib.OW_ERR_STATE
    assert lib.ow_environment_apply_async(None, sky.handle, C.byref(cam), None, rec_dev.data_ptr()) == _lib.OW_ERR_INVALID
    torch.cuda.synchronize()
    assert not rec_dev.any() and not host.tobytes().strip(b"\0")
    for h in (sky, foreign):
        lib.ow_sky_destroy(None, h.handle)          # still the caller's to destroy; touches no freed memory
    live.free()


@pytest.mark.gpu
def test_the_c_example_writes_the_python_wrappers_image(tmp_path):
    """examples/present_host.c at 256^2, a 48 x 32 PPM of 96 x 64 records, 40 steps, 4096 particles, against the wrapper on the same scene"""
    exe = build_example(tmp_path, "present_host")
    ppm = str(tmp_path / "present.ppm")
    r = subprocess.run([exe, ppm, "48", "32", "40", "256", "4096", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    kv = dict(p.split("=") for p in r.stdout.split())
    assert kv["finite"] == "1" and kv["environment_pixels"] == str(96 * 64) and (kv["record_width"], kv["record_height"]) == ("96", "64")
    raw = open(ppm, "rb").read()
    head = b"P6\n48 32\n255\n"
    assert raw.startswith(head) and len(raw) == len(head) + 48 * 32 * 3
    gen, params = make_gen(256, [0, 1, 2])
    sc = scales_of(params)
    spray = gen.spray_create({"amount": 4096})
    bodies = gen.bodies_create(*example_crates())
    for _ in range(40):
        gen.update_all(UPDATE_DELTA, params)
        gen.bodies_step(bodies, sc, 4, UPDATE_DELTA / 4, {"warm_start": True})
        gen.spray_step(spray, UPDATE_DELTA, sc)
    cam = W.camera((0.0, 10.0, -25.0), REF_BASIS, 75.0, 96, 64, 4000.0)
    mesh = gen.mesh_create(*grid(128, 4.0))
    _, bg = gen.mesh_draw(mesh, cam, W.clipmap_origin(cam.position, 4.0), sc, {"falloff": True, "cull_back": True})
    solid = gen.solid_create(*box(CRATE_SHAPE))
    _, mid = gen.solid_draw(solid, bodies, cam, pixels=bg)
    sky = gen.sky_create(example_panorama())
    env = gen.environment_apply(cam, mid, sky)
    m = gen.spray_material_create(*example_textures())
    _, rec = gen.spray_draw(spray, m, cam, pixels=env)
    rgba = gen.present(cam, rec, {"downsample": 2})
    assert np.frombuffer(raw[len(head):], np.uint8).reshape(32, 48, 3).tobytes() == rgba[..., :3].tobytes()
    assert int(kv["sky_pixels"]) == int((((rec["status"] & ENV) != 0) & ((rec["status"] & HIT) == 0)).sum()) > 100
    assert int(kv["crate_pixels"]) == int(((rec["status"] & SOLID) != 0).sum()) and int(kv["sprayed_pixels"]) == int((rec["reserved"][..., 1] > 0).sum())
    for h, fn in ((m, gen.spray_material_destroy), (sky, gen.sky_destroy), (solid, gen.solid_destroy), (mesh, gen.mesh_destroy), (bodies, gen.bodies_destroy),
                  (spray, gen.spray_destroy)):
        fn(h)
    gen.free()

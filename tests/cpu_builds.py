"""The CPU builds of the device headers, and the Python callables over them.

This is the one place that turns tests/<name>/<name>_harness.cpp (the headers of godotoceanwaves_amd/csrc compiled as plain C++, g++
-ffp-contract=off) into a loaded library: one flag list, one build per process and source (harness_library), the argtypes of every entry
point, and the cpu_* functions, Cpu* classes and case writers that feed them.  The *_harness fixtures hand the cached libraries to the tests;
a test module imports the ones its tests take as arguments.  The stand-alone sanitizer programs, every program of examples/ (build_example:
one table, one command) and the layout probes are built here as well.  Scenes and inputs: tests/scenes.py; the comparisons: tests/checks.py."""
import atexit
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from godotoceanwaves_amd.wave_generator import WaveGenerator, WaveGenerator as W
from scenes import (box, calm_maps, camera_words, center_of, f32_options, G, generated_maps, grid, level_camera, look, maps_u16, ray_options,
                    RAY_TOL, RHO, RHO_G, shade_words, SOLID_TWIN_CAM, SPACING, SPRAY_DELTA, SUN, tumbled)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "godotoceanwaves_amd")
CSRC = os.path.join(PKG, "csrc")
INCLUDE = os.path.join(ROOT, "include")


def compile_shared(src, so):
    """a source over the device headers as a shared library: FP32 as written, no contraction"""
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", CSRC, src, "-o", so], check=True)


def harness_source(name):
    return os.path.join(HERE, name, name + "_harness.cpp")


@functools.lru_cache(maxsize=None)
def _build_dir():
    d = tempfile.mkdtemp(prefix="ow_cpu_builds_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


@functools.lru_cache(maxsize=None)
def harness_library(name):
    """tests/<name>/<name>_harness.cpp, built and loaded once per process (the harness sources keep no state between calls)"""
    so = os.path.join(_build_dir(), "lib%s_harness.so" % name)
    compile_shared(harness_source(name), so)
    return C.CDLL(so)


def build_sanitized_harness(name, tmp_path):
    """the harness as a program of its own (its main, under -D<NAME>_HARNESS_MAIN) with the address and undefined-behaviour sanitizers"""
    exe = str(tmp_path / (name + "_harness_main"))
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wno-unknown-pragmas", "-D%s_HARNESS_MAIN" % name.upper(), "-I", CSRC, harness_source(name), "-o", exe], check=True)
    return exe


# the examples: the compiler and warning flags each was written to, and what it links besides the library
_C99, _CXX17 = ["gcc", "-O2", "-std=c99"], ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror"]
_STRICT = _C99 + ["-Wall", "-Wextra", "-pedantic", "-Werror"]
_HIP = ["-L", "/opt/rocm/lib", "-lamdhip64"]
_OWN = [f"-Wl,-rpath,{PKG}", "-Wl,-rpath-link,/opt/rocm/lib"]
_RPATH = [f"-Wl,-rpath,{PKG}", "-Wl,-rpath,/opt/rocm/lib"]
_RPATH_LINK = _RPATH + ["-Wl,-rpath-link,/opt/rocm/lib"]
EXAMPLES = {
    "buoyancy_host": (_STRICT, _HIP + _RPATH_LINK), "floating_bodies_host": (_STRICT, _HIP + _RPATH_LINK),
    "render_host": (_STRICT, _RPATH_LINK), "mesh_host": (_STRICT, _RPATH_LINK), "spray_host": (_STRICT, _RPATH_LINK),
    "spray_draw_host": (_STRICT, _HIP + _RPATH), "solid_draw_host": (_STRICT, _HIP + _RPATH), "present_host": (_STRICT, _HIP + _RPATH),
    "sky_light_host": (_STRICT, _HIP + _RPATH), "shadow_host": (_STRICT, _HIP + _RPATH), "mist_host": (_STRICT, _HIP + _RPATH),
    "mirror_host": (_STRICT, _HIP + _RPATH), "c_consumer": (_STRICT, _OWN), "multi_gpu_host": (_STRICT, _OWN),
    "wave_generator_host": (_CXX17, _OWN), "water_host": (_CXX17 + ["-I", os.path.join(ROOT, "examples")], _OWN),
}


def build_example(tmp_path, name):
    """examples/<name>.c as C99 with -lm, or <name>.cpp as C++17, against the built library"""
    compiler, links = EXAMPLES[name]
    exe = str(tmp_path / name)
    source, libm = (".cpp", []) if compiler[0] == "g++" else (".c", ["-lm"])
    subprocess.run(compiler + ["-I", INCLUDE, os.path.join(ROOT, "examples", name + source), "-o", exe, "-L", PKG, "-locean_waves"] + links + libm,
                   check=True)
    return exe


def layout_probe(tmp_path, name, src, std=("-std=c11", "-Wall", "-Werror")):
    """a C program over ocean_waves.h that prints sizes and offsets: the integers it printed"""
    exe = str(tmp_path / name)
    subprocess.run(["gcc"] + list(std) + ["-I", INCLUDE, "-x", "c", "-", "-o", exe], input=src, text=True, check=True)
    return [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]


QUERY_REC = WaveGenerator.SURFACE_QUERY


@pytest.fixture(scope="module")
def query_harness():
    L = harness_library("query")
    V = C.c_void_p
    L.harness_record_sizes.argtypes = [C.POINTER(C.c_int)] * 3
    L.harness_sample.argtypes = [V, V, C.c_int, C.c_int, V, V, C.c_int, V]
    L.harness_query.argtypes = [V, V, C.c_int, C.c_int, V, V, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float, V]
    L.harness_exp.argtypes = [V, C.c_int, V]
    L.harness_eval.argtypes = [V, C.c_int, C.c_int, V, V, C.c_int, C.c_int, C.c_float, C.c_float, V]
    L.harness_tap.argtypes = [V, C.c_int, C.c_int, V, V]
    return L


def cpu_query(L, disp, norm, scales, xz, max_iterations=0, tolerance=0.0, falloff_center=None):
    """the records the CPU build writes, with the options resolved as the runtime resolves ow_query_options"""
    d, m = maps_u16(disp), maps_u16(norm)
    sc = np.ascontiguousarray(scales, np.float32)
    xz = np.ascontiguousarray(xz, np.float32).reshape(-1, 2)
    out = np.zeros(len(xz), QUERY_REC)
    it = max_iterations if max_iterations > 0 else 16
    tol = tolerance if tolerance > 0 else 1e-3
    cx, cz = falloff_center if falloff_center is not None else (0.0, 0.0)
    L.harness_query(d.ctypes.data, m.ctypes.data, d.shape[1], len(sc), sc.ctypes.data, xz.ctypes.data, len(xz), it, tol,
                    int(falloff_center is not None), cx, cz, out.ctypes.data)
    return out


def cpu_sample(L, disp, norm, scales, xz):
    d, m = maps_u16(disp), maps_u16(norm)
    sc = np.ascontiguousarray(scales, np.float32)
    xz = np.ascontiguousarray(xz, np.float32).reshape(-1, 2)
    out = np.zeros(len(xz), WaveGenerator.SURFACE_SAMPLE)
    L.harness_sample(d.ctypes.data, m.ctypes.data, d.shape[1], len(sc), sc.ctypes.data, xz.ctypes.data, len(xz), out.ctypes.data)
    return out


@pytest.fixture(scope="module")
def raycast_harness():
    L = harness_library("raycast")
    V = C.c_void_p
    L.harness_raycast_sizes.argtypes = [V]
    L.harness_raycast.argtypes = [V, V, C.c_int, C.c_int, V, V, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float, C.c_float,
                                  C.c_float, C.c_float, C.c_int, V, V]
    return L


def cpu_raycast(L, disp, norm, scales, rays, options=None, probe=False):
    """the records of the CPU build, the options resolved as the runtime resolves ow_raycast_options; probe: also the largest |h| each
    ray's samples saw"""
    o = dict(options or {})
    d, m = maps_u16(disp), maps_u16(norm)
    sc = np.ascontiguousarray(scales, np.float32)
    r = np.ascontiguousarray(rays, W.RAY)
    out = np.zeros(len(r), W.RAYCAST_HIT)
    mh = np.zeros(len(r), np.float32)
    center = o.get("falloff_center")
    cx, cz = center if center is not None else (0.0, 0.0)
    L.harness_raycast(d.ctypes.data, m.ctypes.data, d.shape[1], len(sc), sc.ctypes.data, r.ctypes.data, len(r), o.get("max_iterations", 0) or 16,
                      o.get("query_tolerance", 0.0) or 1e-3, int(center is not None), cx, cz, o.get("water_level", 0.0),
                      o.get("sample_spacing", 0.0) or SPACING, o.get("tolerance", 0.0) or RAY_TOL, o.get("max_samples", 0) or 4096, out.ctypes.data,
                      mh.ctypes.data)
    return (out, mh) if probe else out


@pytest.fixture(scope="module")
def buoyancy_harness():
    L = harness_library("buoyancy")
    V = C.c_void_p
    L.harness_buoyancy_sizes.argtypes = [V]
    L.harness_buoyancy.argtypes = [V, C.c_int, C.c_int, V, V, C.c_int, V, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float,
                                   C.c_float, C.c_float, C.c_float, C.c_int, V, V]
    return L


def cpu_buoyancy(L, disp, scales, bodies, hull, options=None, points=None):
    """(results, points) of the CPU build, the options resolved as the runtime resolves ow_buoyancy_options; points: the previous step's
    records (read with warm_start), updated in place"""
    o = dict(options or {})
    d = maps_u16(disp)
    sc = np.ascontiguousarray(scales, np.float32)
    b = np.ascontiguousarray(bodies, W.BUOYANCY_BODY)
    h = np.ascontiguousarray(hull, W.HULL_POINT)
    pts = points if points is not None else np.zeros(len(h), W.BUOYANCY_POINT)
    res = np.zeros(len(b), W.BUOYANCY_RESULT)
    rho = np.float32(o.get("density", 0.0) or RHO)
    g = np.float32(o.get("gravity", 0.0) or G)
    center = o.get("falloff_center")
    cx, cz = center if center is not None else (0.0, 0.0)
    L.harness_buoyancy(d.ctypes.data, d.shape[1], len(sc), sc.ctypes.data, b.ctypes.data, len(b), h.ctypes.data, len(h),
                       o.get("max_iterations", 0) or 16, o.get("tolerance", 0.0) or 1e-3, int(center is not None), cx, cz, float(rho),
                       float(np.float32(rho * g)), o.get("water_level", 0.0), int(bool(o.get("warm_start"))), pts.ctypes.data, res.ctypes.data)
    return res, pts


VELOCITY_REC = W.SURFACE_VELOCITY


@pytest.fixture(scope="module")
def velocity_harness():
    L = harness_library("velocity")
    V = C.c_void_p
    L.harness_velocity_sizes.argtypes = [V]
    L.harness_query_velocity.argtypes = [V, V, C.c_int, C.c_int, V, V, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float, V]
    L.harness_buoyancy_moving.argtypes = [V, V, C.c_int, C.c_int, V, V, C.c_int, V, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float,
                                          C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, V, V]
    return L


def cpu_query_velocity(L, disp, vel, scales, xz, falloff_center=None):
    d, v = maps_u16(disp), maps_u16(vel)
    sc = np.ascontiguousarray(scales, np.float32)
    xz = np.ascontiguousarray(xz, np.float32).reshape(-1, 2)
    out = np.zeros(len(xz), VELOCITY_REC)
    cx, cz = falloff_center if falloff_center is not None else (0.0, 0.0)
    L.harness_query_velocity(d.ctypes.data, v.ctypes.data, d.shape[1], len(sc), sc.ctypes.data, xz.ctypes.data, len(xz), 16, 1e-3,
                             int(falloff_center is not None), cx, cz, out.ctypes.data)
    return out


def cpu_buoyancy_moving(L, disp, vel, scales, bodies, hull, water_level=0.0):
    d, v = maps_u16(disp), maps_u16(vel)
    sc = np.ascontiguousarray(scales, np.float32)
    b = np.ascontiguousarray(bodies, W.BUOYANCY_BODY)
    h = np.ascontiguousarray(hull, W.HULL_POINT)
    pts = np.zeros(len(h), W.BUOYANCY_POINT)
    res = np.zeros(len(b), W.BUOYANCY_RESULT)
    L.harness_buoyancy_moving(d.ctypes.data, v.ctypes.data, d.shape[1], len(sc), sc.ctypes.data, b.ctypes.data, len(b), h.ctypes.data, len(h),
                              16, 1e-3, 0, 0.0, 0.0, RHO, RHO_G, water_level, 0, pts.ctypes.data, res.ctypes.data)
    return res, pts


@pytest.fixture(scope="module")
def bodies_harness():
    L = harness_library("bodies")
    V = C.c_void_p
    L.harness_bodies_sizes.argtypes = [V]
    L.harness_bodies_pose.argtypes = [V, C.c_int, C.c_int, V, V, V]
    L.harness_rigid_pose.argtypes = [V, V]
    L.harness_rigid_finish.argtypes = [V, V, V, C.c_double, C.c_double]
    L.harness_bodies_step.argtypes = [V, V, C.c_int, C.c_int, V, V, C.c_int, V, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float, C.c_float,
                                      C.c_float, C.c_float, C.c_int, C.c_double, C.c_double, C.c_int, V, V, V, V, V, V]
    return L


class CpuSet:
    """what ow_bodies_create leaves on the device, in host memory"""

    def __init__(self, L, state, hull):
        self.L = L
        self.state = np.ascontiguousarray(state, W.RIGID_BODY).copy()
        self.hull = np.ascontiguousarray(hull, W.HULL_POINT)
        self.records = np.zeros(len(self.state), W.BUOYANCY_BODY)
        self.pts = np.zeros(len(self.hull), W.BUOYANCY_POINT)
        self.results = np.zeros(len(self.state), W.BUOYANCY_RESULT)
        self.flags = np.zeros(len(self.state), np.int32)
        L.harness_bodies_pose(self.state.ctypes.data, len(self.state), len(self.hull), self.records.ctypes.data, self.pts.ctypes.data, self.flags.ctypes.data)

    def step(self, disp, scales, substeps, dt, options=None, vel=None, trace=False):
        """the options resolved as the runtime resolves them; returns (per-substep results, per-substep pose records) with trace"""
        o = dict(options or {})
        d = maps_u16(disp)
        v = maps_u16(vel) if vel is not None else None
        sc = np.ascontiguousarray(scales, np.float32)
        rho = np.float32(o.get("density", 0.0) or RHO)
        g = np.float32(o.get("gravity", 0.0) or 9.81)
        center = o.get("falloff_center")
        cx, cz = center if center is not None else (0.0, 0.0)
        tr = np.zeros((substeps, len(self.state)), W.BUOYANCY_RESULT) if trace else None
        tb = np.zeros((substeps, len(self.state)), W.BUOYANCY_BODY) if trace else None
        self.L.harness_bodies_step(d.ctypes.data, v.ctypes.data if v is not None else None, d.shape[1], len(sc), sc.ctypes.data, self.state.ctypes.data,
                                   len(self.state), self.hull.ctypes.data, len(self.hull), o.get("max_iterations", 0) or 16, o.get("tolerance", 0.0) or 1e-3,
                                   int(center is not None), cx, cz, float(rho), float(np.float32(rho * g)), o.get("water_level", 0.0),
                                   int(bool(o.get("warm_start"))), float(g), float(dt), int(substeps), self.records.ctypes.data, self.pts.ctypes.data,
                                   self.results.ctypes.data, self.flags.ctypes.data, tr.ctypes.data if trace else None, tb.ctypes.data if trace else None)
        return tr, tb

    def arrays(self):
        return {"state": self.state.tobytes(), "records": self.records.tobytes(), "results": self.results.tobytes(), "points": self.pts.tobytes()}


@pytest.fixture(scope="module")
def render_harness():
    L = harness_library("render")
    V = C.c_void_p
    L.harness_render_sizes.argtypes = [V]
    L.harness_log.argtypes = [V, C.c_int, V]
    L.harness_pixel_rays.argtypes = [V, C.c_int, C.c_int, V]
    L.harness_render.argtypes = [V, V, C.c_int, C.c_int, V, V, C.c_int, C.c_int, V, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float, C.c_float,
                                 C.c_float, C.c_float, C.c_int, V, V]
    return L


def cpu_render(L, disp, norm, scales, cam, options=None):
    """(rgba [H][W][4], records [H][W]) of the CPU build, the options resolved as the runtime resolves them"""
    o = ray_options(options, cam)
    d, m = maps_u16(disp), maps_u16(norm)
    sc = np.ascontiguousarray(scales, np.float32)
    cw, sw = camera_words(cam), shade_words(options)
    rgba = np.zeros((cam.height, cam.width, 4), np.uint8)
    rec = np.zeros((cam.height, cam.width), W.RENDER_PIXEL)
    center = o.get("falloff_center")
    cx, cz = center if center is not None else (0.0, 0.0)
    L.harness_render(d.ctypes.data, m.ctypes.data, d.shape[1], len(sc), sc.ctypes.data, cw.ctypes.data, cam.width, cam.height, sw.ctypes.data,
                     o.get("max_iterations", 0) or 16, o.get("query_tolerance", 0.0) or 1e-3, int(center is not None), cx, cz,
                     o.get("water_level", 0.0), o.get("sample_spacing", 0.0) or SPACING, o.get("tolerance", 0.0) or RAY_TOL,
                     o.get("max_samples", 0) or 4096, rgba.ctypes.data, rec.ctypes.data)
    return rgba, rec


@pytest.fixture(scope="module")
def mesh_harness():
    L = harness_library("mesh")
    V, I, F = C.c_void_p, C.c_int, C.c_float
    L.harness_mesh_sizes.argtypes = [V]
    L.harness_mesh_vertices.argtypes = [V, I, I, V, V, I, V, I, F, F, V, V]
    L.harness_mesh_draw.argtypes = [V, V, I, I, V, V, I, V, I, V, V, I, I, V, I, F, F, F, I, I, V, V, V, V, V]
    L.harness_mesh_cover_all.argtypes = L.harness_mesh_draw.argtypes + [V]
    L.harness_mesh_setups.argtypes = L.harness_mesh_draw.argtypes[:20] + [V]
    return L


SETUP = np.dtype([("kind", np.int32), ("x0", np.int32), ("x1", np.int32), ("y0", np.int32), ("y1", np.int32)])   # a triangle's set-up, as the harnesses return it
COVER = np.dtype([("covered", np.int32), ("outside", np.int32)])   # a brute pass's count per triangle: centres covered, and of those outside its box


def cpu_mesh_draw(L, disp, norm, scales, mesh, origin, cam, options=None, brute=False):
    """the CPU build's draw: dict of vertices, vis [H][W] uint64, rgba [H][W][4], rec [H][W], counters (skipped, culled, per_lane, cooperative).
    brute: harness_mesh_cover_all, every centre of the picture instead of the set-up's box, and `cover` and `setups` per triangle;
    brute="setups": the set-ups alone, nothing drawn"""
    o = options or {}
    d, m = maps_u16(disp), maps_u16(norm)
    sc = np.ascontiguousarray(scales, np.float32)
    v = np.ascontiguousarray(mesh[0], np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(mesh[1], np.int32).reshape(-1, 3)
    org = np.ascontiguousarray(origin, np.float32)
    center = center_of(o, cam)
    cx, cz = center if center is not None else (0.0, 0.0)
    cw, sw = camera_words(cam), shade_words(o)
    out = dict(vertices=np.zeros(len(v), W.MESH_VERTEX), vis=np.zeros((cam.height, cam.width), np.uint64),
               rgba=np.zeros((cam.height, cam.width, 4), np.uint8), rec=np.zeros((cam.height, cam.width), W.RENDER_PIXEL), counters=np.zeros(4, np.uint32))
    inputs = (d.ctypes.data, m.ctypes.data, d.shape[1], len(sc), sc.ctypes.data, v.ctypes.data, len(v), t.ctypes.data, len(t), org.ctypes.data,
              cw.ctypes.data, cam.width, cam.height, sw.ctypes.data, int(center is not None), cx, cz, float(o.get("near", 0.0)),
              int(bool(o.get("cull_back"))), int(o.get("lane_box", 0)))
    outputs = (out["vertices"].ctypes.data, out["vis"].ctypes.data, out["rgba"].ctypes.data, out["rec"].ctypes.data, out["counters"].ctypes.data)
    if not brute:
        L.harness_mesh_draw(*inputs, *outputs)
        return out
    out.update(cover=np.zeros(len(t), COVER), setups=np.zeros(len(t), SETUP))
    L.harness_mesh_setups(*inputs, out["setups"].ctypes.data)
    if brute != "setups":
        L.harness_mesh_cover_all(*inputs, *outputs, out["cover"].ctypes.data)
    return out


@pytest.fixture(scope="module")
def spray_harness():
    L = harness_library("spray")
    V, I, F, D = C.c_void_p, C.c_int, C.c_float, C.c_double
    L.harness_spray_sizes.argtypes = [V]
    L.harness_spray_defaults.argtypes = [V]
    L.harness_hash32.argtypes = [V, I, V]
    L.harness_exp_impulse.argtypes = [V, I, F, V]
    L.harness_log.argtypes = [V, I, V]
    L.harness_spray_create.argtypes = [V, C.POINTER(C.c_char_p)]
    L.harness_spray_create.restype = V
    L.harness_spray_destroy.argtypes = [V]
    L.harness_spray_params.argtypes = [V, V, V, V]
    L.harness_spray_step.argtypes = [V, D, V, V, I, I, V, V]
    L.harness_spray_clock.argtypes = [V, V, V]
    L.harness_spray_read.argtypes = [V, V, V, V, V]
    L.harness_spray_stats.argtypes = [V, V, V]
    return L


class CpuEmitter:
    """the CPU build's emitter over fixed maps; step() returns the step's records"""

    def __init__(self, L, opts, disp, norm, scales):
        self.L, self.opts = L, opts
        why = C.c_char_p()
        self.h = L.harness_spray_create(C.byref(opts), C.byref(why))
        assert self.h, why.value
        self.amount = opts.amount
        self.set_maps(disp, norm, scales)
        t, E, axis = C.c_uint32(), np.zeros((3, 4), np.float32), np.zeros((3, 3), np.float32)
        L.harness_spray_params(self.h, C.byref(t), E.ctypes.data, axis.ctypes.data)
        self.P = dict(amount=opts.amount, t=t.value, seed=opts.random_seed, emitter_lifetime=opts.emitter_lifetime, lifetime=opts.lifetime,
                      randomness=opts.lifetime_randomness, particle_scale=tuple(opts.particle_scale), E=E, axis=axis)

    def set_maps(self, disp, norm, scales):
        self.d, self.m, self.sc = maps_u16(disp), maps_u16(norm), np.ascontiguousarray(scales, np.float32)

    def step(self, delta=SPRAY_DELTA):
        restarted = np.zeros(self.amount, np.uint8)
        assert self.L.harness_spray_step(self.h, delta, self.d.ctypes.data, self.m.ctypes.data, self.d.shape[1], len(self.sc), self.sc.ctypes.data,
                                         restarted.ctypes.data) == 0
        out = self.read()
        f3, u3 = np.zeros(3, np.float32), np.zeros(3, np.uint32)
        self.L.harness_spray_clock(self.h, f3.ctypes.data, u3.ctypes.data)
        out.update(restarted=restarted.astype(bool),
                   clock=dict(time=f3[0], prev=f3[1], phase=f3[2], utime=int(u3[0]), wrapped=int(u3[1]), base=int(u3[2])))
        return out

    def read(self):
        inst, part = np.zeros(self.amount, W.SPRAY_INSTANCE), np.zeros(self.amount, W.SPRAY_PARTICLE)
        draw, live = np.zeros(self.amount, np.uint32), C.c_uint32()
        self.L.harness_spray_read(self.h, inst.ctypes.data, part.ctypes.data, draw.ctypes.data, C.byref(live))
        return dict(instances=inst, particles=part, draw=draw[:live.value].copy(), live=live.value)

    def stats(self):
        t, four = C.c_double(), (C.c_uint64 * 4)()
        self.L.harness_spray_stats(self.h, C.byref(t), four)
        return dict(time=t.value, steps=four[0], restarts=four[1], spawned=four[2], rejected=four[3])

    def close(self):
        if self.h:
            self.L.harness_spray_destroy(self.h)
        self.h = None

    __del__ = close


BILLBOARD_CASE = np.dtype([("width", np.int32), ("height", np.int32), ("cam", np.float32, 15), ("count", np.int32), ("live", np.int32), ("has_list", np.int32),
                 ("time", np.float32), ("foam", np.float32, 3), ("max_alpha", np.float32), ("aw", np.int32), ("ah", np.int32), ("asrgb", np.int32),
                 ("dw", np.int32), ("dh", np.int32), ("dsrgb", np.int32), ("near", np.float32), ("background", np.float32, 3),
                 ("bin_side", np.int32), ("has_pixels", np.int32)])


@pytest.fixture(scope="module")
def billboard_harness():
    L = harness_library("spray_draw")
    V, I = C.c_void_p, C.c_int
    L.harness_billboard_sizes.argtypes = [V]
    L.harness_srgb_table.argtypes = [V]
    L.harness_billboard_draw.argtypes = [V, V, V, V, V, V, V, V, V]
    L.harness_billboard_fragment.argtypes = [V, V, V, V, I, I, C.c_float, C.c_int32, V]
    return L


def billboard_case_of(cam, count, mat, time=0.0, order=None, opts=None, records=None):
    o = opts or {}
    h = np.zeros(1, BILLBOARD_CASE)
    h["width"], h["height"], h["cam"] = cam.width, cam.height, camera_words(cam)
    h["count"], h["live"], h["has_list"], h["time"] = count, 0 if order is None else len(order), int(order is not None), time
    h["foam"], h["max_alpha"] = mat["foam_color"], mat["max_alpha"]
    h["ah"], h["aw"], h["asrgb"] = mat["albedo"].shape[0], mat["albedo"].shape[1], mat.get("albedo_srgb", 1)
    h["dh"], h["dw"], h["dsrgb"] = mat["dissolve"].shape[0], mat["dissolve"].shape[1], mat.get("dissolve_srgb", 1)
    h["near"], h["background"], h["bin_side"] = o.get("near", 0.0), o.get("background_color", (0, 0, 0)), o.get("bin_side", 0)
    h["has_pixels"] = int(records is not None)
    return h


def billboard_case_arrays(inst, mat, order, records):
    inst = np.ascontiguousarray(inst, W.SPRAY_INSTANCE).reshape(-1)
    lst = np.ascontiguousarray(order if order is not None else [], np.uint32)
    a, d = np.ascontiguousarray(mat["albedo"], np.uint8), np.ascontiguousarray(mat["dissolve"], np.uint8)
    rec = np.array(records, W.RENDER_PIXEL, copy=True, order="C") if records is not None else None
    return inst, lst, a, d, rec


def cpu_billboard_draw(L, inst, cam, mat, time=0.0, order=None, opts=None, records=None):
    """the CPU build's draw: dict of rgba [H][W][4], rec [H][W] or None, drawn, culled, bins (side, nx, ny, words)"""
    inst, lst, a, d, rec = billboard_case_arrays(inst, mat, order, records)
    h = billboard_case_of(cam, len(inst), mat, time, order, opts, records)
    rgba = np.zeros((cam.height, cam.width, 4), np.uint8)
    counters, bins = np.zeros(2, np.uint32), np.zeros(4, np.int32)
    L.harness_billboard_draw(h.ctypes.data, inst.ctypes.data, lst.ctypes.data, a.ctypes.data, d.ctypes.data, rec.ctypes.data if rec is not None else None,
                             rgba.ctypes.data, counters.ctypes.data, bins.ctypes.data)
    return dict(rgba=rgba, rec=rec, drawn=int(counters[0]), culled=int(counters[1]), bins=tuple(int(b) for b in bins))


SOLID_DEFAULTS = dict(color=(0.45, 0.30, 0.15), light_direction=SUN, light_color=(1.0, 1.0, 1.0), ambient_color=(0.05, 0.08, 0.10), background_color=(0.0, 0.0, 0.0))


SOLID_CASE = np.dtype([("width", np.int32), ("height", np.int32), ("cam", np.float32, 15), ("num_vertices", np.int32), ("num_triangles", np.int32),
                 ("count", np.int32), ("stride", np.int32), ("has_flags", np.int32), ("near", np.float32), ("color", np.float32, 3),
                 ("light_direction", np.float32, 3), ("light_color", np.float32, 3), ("ambient_color", np.float32, 3),
                 ("background_color", np.float32, 3), ("two_sided", np.int32), ("lane_box", np.int32), ("has_pixels", np.int32)])


@pytest.fixture(scope="module")
def solid_harness():
    L = harness_library("solid")
    V = C.c_void_p
    L.harness_solid_sizes.argtypes = [V]
    L.harness_solid_draw.argtypes = [V] * 9
    L.harness_solid_cover_all.argtypes = [V] * 10
    L.harness_solid_setups.argtypes = [V] * 6
    return L


def solid_case_of(cam, shape, count, opts=None, records=None, stride=12, flags=None):
    o = dict(SOLID_DEFAULTS)
    o.update(opts or {})
    h = np.zeros(1, SOLID_CASE)
    h["width"], h["height"], h["cam"] = cam.width, cam.height, camera_words(cam)
    h["num_vertices"], h["num_triangles"], h["count"], h["stride"], h["has_flags"] = len(shape[0]), len(shape[1]), count, stride, int(flags is not None)
    h["near"], h["two_sided"], h["lane_box"] = o.get("near", 0.0), int(bool(o.get("two_sided"))), o.get("lane_box", 0)
    for k in ("color", "light_direction", "light_color", "ambient_color", "background_color"):
        h[k] = o[k]
    h["has_pixels"] = int(records is not None)
    return h


def solid_case_arrays(shape, tf, records, flags=None):
    v = np.ascontiguousarray(shape[0], np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(shape[1], np.int32).reshape(-1, 3)
    tf = np.ascontiguousarray(tf, np.float32)
    fl = np.ascontiguousarray(flags, np.int32) if flags is not None else None
    rec = np.array(records, W.RENDER_PIXEL, copy=True, order="C") if records is not None else None
    return v, t, tf, fl, rec


def cpu_solid_draw(L, shape, tf, cam, opts=None, records=None, stride=12, flags=None, brute=False):
    """the CPU build's draw: dict of rgba [H][W][4], rec [H][W] or None, vis [H][W], skipped, culled, lane, wave, drawn.  brute:
    harness_solid_cover_all, every centre of the picture instead of the set-up's box, and `cover` and `setups` per (instance, triangle) pair;
    brute="setups": the set-ups alone"""
    v, t, tf, fl, rec = solid_case_arrays(shape, tf, records, flags)
    count = tf.size // stride
    h = solid_case_of(cam, (v, t), count, opts, records, stride, fl)
    rgba = np.zeros((cam.height, cam.width, 4), np.uint8)
    vis = np.zeros((cam.height, cam.width), np.uint64)
    counters = np.zeros(4, np.uint32)
    inputs = (h.ctypes.data, v.ctypes.data, t.ctypes.data, tf.ctypes.data if tf.size else None, fl.ctypes.data if fl is not None else None)
    outputs = (rec.ctypes.data if rec is not None else None, rgba.ctypes.data, counters.ctypes.data, vis.ctypes.data)
    extra = {}
    if brute:
        extra = dict(cover=np.zeros(count * len(t), COVER), setups=np.zeros(count * len(t), SETUP))
        L.harness_solid_setups(*inputs, extra["setups"].ctypes.data)
        if brute == "setups":
            return extra
        L.harness_solid_cover_all(*inputs, *outputs, extra["cover"].ctypes.data)
    else:
        L.harness_solid_draw(*inputs, *outputs)
    s, c, ln, wv = (int(x) for x in counters)
    return dict(rgba=rgba, rec=rec, vis=vis, skipped=s, culled=c, lane=ln, wave=wv, drawn=ln + wv, **extra)


def calm_picture(mesh_harness, cam):
    d, m, sc = calm_maps()
    return cpu_mesh_draw(mesh_harness, d, m, sc, grid(16, 8.0), (0.0, 0.0, 0.0), cam)["rec"]


def twin_scene(mesh_harness):
    cam = look(**SOLID_TWIN_CAM)
    return box((2.5, 2.5, 2.5)), tumbled(7, seed=20261018), cam, calm_picture(mesh_harness, cam)


ENV_DEFAULTS = dict(fog_mode=1, density=1.0, depth_begin=200.0, depth_end=350.0, depth_curve=0.25, aerial_perspective=0.626, sun_scatter=0.05,
                    light_color=(0.272954, 0.419272, 0.484632), sun_color=(1.0, 1.0, 1.0), sun_direction=SUN, sky_color=(0.25, 0.40, 0.60))


PRESENT_DEFAULTS = dict(downsample=1, tonemap=2, exposure=1.0, white=1.0, srgb=1, brightness=0.85, contrast=1.07, saturation=1.5)


ENV_CASE = np.dtype([("width", np.int32), ("height", np.int32), ("cam", np.float32, 15), ("fog_mode", np.int32), ("density", np.float32),
                     ("depth_begin", np.float32), ("depth_end", np.float32), ("depth_curve", np.float32), ("aerial_perspective", np.float32),
                     ("sun_scatter", np.float32), ("light_color", np.float32, 3), ("sun_color", np.float32, 3), ("sun_direction", np.float32, 3),
                     ("sky_color", np.float32, 3), ("has_sky", np.int32), ("sky_width", np.int32), ("sky_height", np.int32), ("sky_srgb", np.int32),
                     ("energy", np.float32)])


PRESENT_CASE = np.dtype([("width", np.int32), ("height", np.int32), ("downsample", np.int32), ("tonemap", np.int32), ("exposure", np.float32),
                         ("white", np.float32), ("srgb", np.int32), ("brightness", np.float32), ("contrast", np.float32), ("saturation", np.float32)])


@pytest.fixture(scope="module")
def env_harness():
    L = harness_library("environment")
    V, I = C.c_void_p, C.c_int
    L.harness_environment_sizes.argtypes = [V]
    L.harness_atan2.argtypes = [V, V, I, V]
    L.harness_acos.argtypes = [V, I, V]
    L.harness_sky_lookup.argtypes = [V, V, V, I, V]
    L.harness_fog_amount.argtypes = [V, V, I, V]
    L.harness_environment_apply.argtypes = [V, V, V, V]
    L.harness_present.argtypes = [V, V, V, V, V]
    return L


def env_case(cam, opts=None, sky=None):
    o = f32_options(ENV_DEFAULTS, opts)
    h = np.zeros(1, ENV_CASE)
    h["width"], h["height"], h["cam"] = cam.width, cam.height, camera_words(cam)
    for k in ENV_DEFAULTS:
        h[k] = o[k]
    if sky is not None:
        h["has_sky"], h["sky_height"], h["sky_width"], h["sky_srgb"], h["energy"] = 1, sky["image"].shape[0], sky["image"].shape[1], sky["srgb"], sky["energy"]
    return h


def present_case(width, height, opts=None):
    o = f32_options(PRESENT_DEFAULTS, opts)
    h = np.zeros(1, PRESENT_CASE)
    h["width"], h["height"] = width, height
    for k in PRESENT_DEFAULTS:
        h[k] = o[k]
    return h


def cpu_environment(L, records, cam, opts=None, sky=None):
    """the CPU build's pass: dict of rec (a copy, rewritten) and the stages ray, sky, amount, fog"""
    rec = np.array(records, W.RENDER_PIXEL, copy=True, order="C")
    assert rec.shape == (cam.height, cam.width)
    h = env_case(cam, opts, sky)
    st = np.zeros((cam.height, cam.width, 10), np.float32)
    L.harness_environment_apply(h.ctypes.data, sky["image"].ctypes.data if sky is not None else None, rec.ctypes.data, st.ctypes.data)
    return dict(rec=rec, ray=st[..., 0:3], sky=st[..., 3:6], amount=st[..., 6], fog=st[..., 7:10])


def cpu_present(L, records, opts=None):
    """the CPU build's present: dict of rgba [H / s][W / s][4], linear [H / s][W / s][4] and the stages exposed, mapped, encoded, adjusted"""
    rec = np.ascontiguousarray(records, W.RENDER_PIXEL)
    hh, ww = rec.shape
    o = f32_options(PRESENT_DEFAULTS, opts)
    s = max(o["downsample"], 1)
    h = present_case(ww, hh, opts)
    rgba = np.zeros((hh // s, ww // s, 4), np.uint8)
    lin = np.zeros((hh // s, ww // s, 4), np.float32)
    st = np.zeros((hh // s, ww // s, 12), np.float32)
    L.harness_present(h.ctypes.data, rec.ctypes.data, rgba.ctypes.data, lin.ctypes.data, st.ctypes.data)
    return dict(rgba=rgba, linear=lin, exposed=st[..., 0:3], mapped=st[..., 3:6], encoded=st[..., 6:9], adjusted=st[..., 9:12])


def sky_lookup(L, sky, dirs):
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    out = np.zeros((len(d), 3), np.float32)
    L.harness_sky_lookup(env_case(level_camera(4, 4), None, sky).ctypes.data, sky["image"].ctypes.data, d.ctypes.data, len(d), out.ctypes.data)
    return out


PICTURE_CAM = dict(position=(0.0, 20.0, 0.0), yaw_deg=15.0, pitch_deg=-1.5, fov=60.0, width=72, height=36, max_distance=4000.0)


@functools.lru_cache(maxsize=None)
def _pictures(mesh_harness):
    cam = look(**PICTURE_CAM)
    d, m, sc = calm_maps()
    calm = cpu_mesh_draw(mesh_harness, d, m, sc, grid(64, 16.0), (0.0, 0.0, 0.0), cam)
    d, m, sc = generated_maps(128, [0, 1, 2], ticks=3)
    sea = cpu_mesh_draw(mesh_harness, d, m, sc, grid(64, 16.0), W.clipmap_origin(cam.position, 16.0), cam, {"falloff": True})
    for a in (calm["rec"], calm["rgba"], sea["rec"], sea["rgba"]):
        a.setflags(write=False)
    return dict(cam=cam, calm=dict(rec=calm["rec"], rgba=calm["rgba"]), sea=dict(rec=sea["rec"], rgba=sea["rgba"]))


@pytest.fixture(scope="module")
def pictures(mesh_harness):
    """ow_mesh_draw's CPU build over a calm sea (a 1 km grid: hits from a few metres to beyond the fog's end, and the sky above the horizon)
    and over a generated one (128^2 x 3 oracle maps, the shader's falloff): drawn once per process and shared, so read-only"""
    return _pictures(mesh_harness)


RADIANCE_DEFAULTS = dict(levels=6, samples=64, base_width=1024)


LIGHT_DEFAULTS = dict(ambient_energy=1.0, reflection_energy=1.0, specular=0.5)


RADIANCE_CASE = np.dtype([("sky_width", np.int32), ("sky_height", np.int32), ("sky_srgb", np.int32), ("energy", np.float32), ("levels", np.int32),
                          ("samples", np.int32), ("base_width", np.int32)])


LIGHT_CASE = np.dtype([("width", np.int32), ("height", np.int32), ("cam", np.float32, 15), ("ambient_energy", np.float32),
                       ("reflection_energy", np.float32), ("specular", np.float32)])


STAGES = (("view", 0, 3), ("reflect", 3, 6), ("lod", 6, 7), ("radiance", 7, 10), ("env", 10, 12), ("irradiance", 12, 15), ("ambient", 15, 18), ("spec", 18, 21))


@pytest.fixture(scope="module")
def sky_harness():
    L = harness_library("sky_light")
    V, I = C.c_void_p, C.c_int
    L.harness_sky_light_sizes.argtypes = [V]
    L.harness_radiance_plan.argtypes = [I, I, I, I, V]
    L.harness_radiance_dir_table.argtypes = [I, I, V]
    L.harness_radiance_sample_table.argtypes = [C.c_double, I, V]
    L.harness_radiance_new.argtypes = [V, V]
    L.harness_radiance_new.restype = V
    L.harness_radiance_free.argtypes = [V]
    L.harness_radiance_get.argtypes = [V, I, I, V, V]
    L.harness_radiance_lookup.argtypes = [V, I, I, V, I, V]
    L.harness_sky_light_apply.argtypes = [V, V, V, V]
    return L


def radiance_case(sky, opts=None):
    o = dict(RADIANCE_DEFAULTS, **(opts or {}))
    h = np.zeros(1, RADIANCE_CASE)
    h["sky_height"], h["sky_width"], h["sky_srgb"], h["energy"] = sky["image"].shape[0], sky["image"].shape[1], sky["srgb"], sky["energy"]
    for k in RADIANCE_DEFAULTS:
        h[k] = o[k] or RADIANCE_DEFAULTS[k]
    return h


def light_case(cam, opts=None):
    o = f32_options(LIGHT_DEFAULTS, opts)
    h = np.zeros(1, LIGHT_CASE)
    h["width"], h["height"], h["cam"] = cam.width, cam.height, camera_words(cam)
    for k in LIGHT_DEFAULTS:
        h[k] = o[k]
    return h


class CpuPyramid:
    """the CPU build's pyramid of a sky (sky_of's dict): R[k], M[k], E as (h, w, 4) float32, lookups and the pass"""

    def __init__(self, L, sky, opts=None):
        self.L, self.sky = L, sky
        self.case = radiance_case(sky, opts)
        self.levels = int(self.case["levels"][0])
        self.ptr = L.harness_radiance_new(self.case.ctypes.data, sky["image"].ctypes.data)
        assert self.ptr, "the sizes are refused"

    def __del__(self):
        if getattr(self, "ptr", None):
            self.L.harness_radiance_free(self.ptr)

    def texture(self, kind, k=0):
        size = (C.c_int * 2)()
        if not self.L.harness_radiance_get(self.ptr, kind, k, size, None):
            return None
        out = np.zeros((size[1], size[0], 4), np.float32)
        self.L.harness_radiance_get(self.ptr, kind, k, size, out.ctypes.data)
        return out

    R = lambda self, k: self.texture(0, k)    # noqa: E731
    M = lambda self, k: self.texture(1, k)    # noqa: E731
    E = property(lambda self: self.texture(2))

    def lookup(self, kind, k, dirs):
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        out = np.zeros_like(d)
        self.L.harness_radiance_lookup(self.ptr, kind, k, d.ctypes.data, len(d), out.ctypes.data)
        return out

    def apply(self, records, cam, opts=None):
        """dict of rec (a copy, rewritten) and the stages"""
        rec = np.array(records, W.RENDER_PIXEL, copy=True, order="C")
        assert rec.shape == (cam.height, cam.width)
        h = light_case(cam, opts)
        st = np.zeros((cam.height, cam.width, 21), np.float32)
        self.L.harness_sky_light_apply(self.ptr, h.ctypes.data, rec.ctypes.data, st.ctypes.data)
        out = dict(rec=rec)
        for name, a, b in STAGES:
            out[name] = st[..., a] if b == a + 1 else st[..., a:b]
        return out


@pytest.fixture(scope="module")
def shadow_harness():
    L = harness_library("shadow")
    V, I = C.c_void_p, C.c_int
    L.harness_shadow_sizes.argtypes = [V]
    L.harness_shadow_frame.argtypes = [V, I, V]
    L.harness_shadow_clear.argtypes = [I, V, V]
    L.harness_shadow_cast.argtypes = [V, I, V, I, V, I, V, I, V, I, V, V, V]
    L.harness_shadow_apply.argtypes = [V, I, V, I, V, I, I, V, V, V]
    L.harness_shadow_cover_all.argtypes = L.harness_shadow_cast.argtypes + [V]
    L.harness_shadow_setups.argtypes = L.harness_shadow_cast.argtypes[:10] + [V]
    return L


def cpu_shadow_cast(L, frame, size, shape, tf, brute=False):
    """one cast of the CPU build into a cleared map: dict of map [size][size] uint32, skipped, culled, lane, wave, drawn.  brute:
    harness_shadow_cover_all, every centre of the map instead of the set-up's box and whatever the depths, and `cover` and `setups` per
    (instance, triangle) pair; brute="setups": the set-ups alone"""
    v = np.ascontiguousarray(shape[0], np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(shape[1], np.int32).reshape(-1, 3)
    tf = np.ascontiguousarray(tf, np.float32).reshape(-1, 12)
    fr = W.shadow_frame(frame)
    words, counters = np.zeros((size, size), np.uint32), np.zeros(4, np.uint32)
    L.harness_shadow_clear(size, words.ctypes.data, counters.ctypes.data)
    inputs = (C.addressof(fr), size, v.ctypes.data, len(v), t.ctypes.data, len(t), tf.ctypes.data if tf.size else None, 12, None, len(tf))
    extra = {}
    if brute:
        extra = dict(cover=np.zeros(len(tf) * len(t), COVER), setups=np.zeros(len(tf) * len(t), SETUP))
        L.harness_shadow_setups(*inputs, extra["setups"].ctypes.data)
        if brute == "setups":
            return extra
        L.harness_shadow_cover_all(*inputs, words.ctypes.data, counters.ctypes.data, None, extra["cover"].ctypes.data)
    else:
        L.harness_shadow_cast(*inputs, words.ctypes.data, counters.ctypes.data, None)
    s, c, ln, wv = (int(x) for x in counters)
    return dict(map=words, skipped=s, culled=c, lane=ln, wave=wv, drawn=ln + wv, **extra)


def build_scene_dump(tmp_path):
    """tests/example_scene/scene_dump.c over examples/scene.h: a program of its own under the sanitizers, nothing of the library linked"""
    exe = str(tmp_path / "scene_dump")
    subprocess.run(["gcc", "-O1", "-g", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", INCLUDE, os.path.join(HERE, "example_scene", "scene_dump.c"), "-o", exe, "-lm"], check=True)
    return exe

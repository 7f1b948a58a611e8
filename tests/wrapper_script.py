"""What tests/golden/wrapper_surface.json records of the Python wrapper (godotoceanwaves_amd/wave_generator.py, group.py and the modules they are
assembled from), for scripts/record_wrapper_surface.py to write and tests/test_wrapper_surface.py to compare:

  surface()  the names WaveGenerator, WaveGeneratorGroup and WaveCascadeParameters expose, every callable's signature, every dtype, every constant
  options()  each dict-to-struct converter and each static helper on a fixed list of inputs: the struct's bytes, or the exception's type and text
  traces()   the library calls each wrapper method makes, on a stand-in library that records name and arguments and answers OW_OK

It needs the built library for the *_default entry points only, and no GPU.
"""
import ctypes as C
import inspect
import json

import numpy as np

from godotoceanwaves_amd import _lib, wave_generator as wg
from godotoceanwaves_amd.group import WaveGeneratorGroup
from godotoceanwaves_amd.wave_generator import WaveCascadeParameters, WaveGenerator as W

PLAIN = {"__dict__", "__module__", "__weakref__", "__doc__"} | set(dir(object))


def plain(v):
    """a value as JSON holds it (tuples are lists there)"""
    return json.loads(json.dumps(v))


def show(v):
    """a result in a form JSON holds: bytes for structs and arrays, type and text for an exception"""
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, (np.integer, np.floating)):
        return {"scalar": str(v.dtype), "value": v.item()}
    if isinstance(v, BaseException):
        return {"error": type(v).__name__, "text": str(v)}
    if isinstance(v, (C.Structure, C.Array)):
        return {"struct": type(v).__name__, "bytes": bytes(v).hex()}
    if isinstance(v, np.ndarray):
        return {"dtype": str(v.dtype) if v.dtype.names is None else plain(v.dtype.descr), "shape": list(v.shape), "bytes": v.tobytes().hex()}
    if isinstance(v, (tuple, list)):
        return [show(x) for x in v]
    if isinstance(v, dict):
        return {str(k): show(x) for k, x in v.items()}
    return {"object": type(v).__name__, "fields": {k: show(x) for k, x in sorted(vars(v).items())}}


def attempt(fn, *a, **kw):
    try:
        return show(fn(*a, **kw))
    except Exception as e:   # the exception is the recorded result
        return show(e)


# ---- 1. the surface ------------------------------------------------------------------------------------------------------------------------
def surface():
    out = {}
    for cls in (W, WaveGeneratorGroup, WaveCascadeParameters):
        names = sorted(n for n in dir(cls) if n not in PLAIN)
        rec = {"names": names, "instance": sorted(vars(cls())), "callables": {}, "properties": [], "dtypes": {}, "constants": {}}
        for n in names:
            static, v = inspect.getattr_static(cls, n), getattr(cls, n)
            if isinstance(static, property):
                rec["properties"].append(n)
            elif isinstance(v, np.dtype):
                rec["dtypes"][n] = {"descr": plain(v.descr), "itemsize": v.itemsize}
            elif callable(v):
                rec["callables"][n] = [type(static).__name__, str(inspect.signature(v))]
            else:
                rec["constants"][n] = plain({str(k): x for k, x in v.items()} if isinstance(v, dict) else v)
        out[cls.__name__] = rec
    out["wave_generator"] = sorted(n for n in ("WaveGenerator", "WaveCascadeParameters", "Sky", "Radiance", "ShadowMap", "_addr", "_ref", "_scales",
                                               "_check_device_size", "G", "DEPTH", "_BodySet", "_Mesh", "_Spray", "_SprayMaterial", "_Solid", "_Descriptor")
                                   if hasattr(wg, n))
    out["G_DEPTH"] = [wg.G, wg.DEPTH]
    return out


# ---- 2. the option converters ----------------------------------------------------------------------------------------------------------------
def cam(width=6, height=4, position=(3.0, 5.0, -7.0)):
    return W.camera(position, np.eye(3), 60.0, width, height, 100.0)


QUERY = {"max_iterations": 7, "tolerance": 0.002, "falloff_center": (3.5, -4.25)}
BUOYANCY = dict(QUERY, density=1000.5, gravity=9.75, water_level=0.5, warm_start=True, water_velocity=True)
RAYCAST = {"water_level": 0.25, "sample_spacing": 0.125, "tolerance": 0.004, "max_samples": 99, "query_tolerance": 0.003, "max_iterations": 9,
           "falloff_center": (1.5, 2.5)}
MATERIAL = {"water_color": (0.1, 0.2, 0.3), "foam_color": (0.9, 0.8, 0.7), "roughness": 0.35, "normal_strength": 1.5, "light_direction": (0.0, 0.6, 0.8),
            "light_color": (1.0, 0.9, 0.8), "ambient_color": (0.05, 0.06, 0.07), "sky_color": (0.3, 0.4, 0.5)}
# converter -> (the struct it makes, every allowed key with a value that is not the default, whether it takes the camera)
CONVERTERS = {
    "query_options": (_lib.ow_query_options, QUERY, False),
    "buoyancy_options": (_lib.ow_buoyancy_options, BUOYANCY, False),
    "bodies_options": (_lib.ow_bodies_options, BUOYANCY, False),
    "raycast_options": (_lib.ow_raycast_options, RAYCAST, False),
    "render_options": (_lib.ow_render_options, dict(MATERIAL, falloff=True, **RAYCAST), True),
    "mesh_options": (_lib.ow_mesh_options, dict(MATERIAL, near=0.125, cull_back=True, lane_box=12, falloff=True, falloff_center=(8.0, 9.0)), True),
    "spray_options": (_lib.ow_spray_options, {"amount": 64, "num_particles": 3, "emitter_lifetime": 2.5, "lifetime": 1.25, "lifetime_randomness": 0.5,
                                              "particle_scale": (1.0, 2.0, 3.0), "random_seed": 77, "emission_transform": np.arange(12.0).reshape(3, 4),
                                              "start_time": 3.75}, False),
    "spray_material_options": (_lib.ow_billboard_material_options, {"foam_color": (0.5, 0.25, 0.125), "max_alpha": 0.75, "albedo_srgb": 0,
                                                                    "dissolve_srgb": 0}, False),
    "spray_draw_options": (_lib.ow_billboard_draw_options, {"near": 0.25, "background_color": (0.1, 0.2, 0.3), "bin_side": 16}, False),
    "solid_options": (_lib.ow_solid_options, {"near": 0.5, "color": (0.2, 0.3, 0.4), "light_direction": (0.6, 0.8, 0.0), "light_color": (0.9, 0.8, 0.7),
                                              "ambient_color": (0.01, 0.02, 0.03), "background_color": (0.5, 0.6, 0.7), "two_sided": True, "lane_box": 20}, False),
    "sky_options": (_lib.ow_sky_options, {"srgb": 0, "energy": 2.5}, False),
    "environment_options": (_lib.ow_environment_options, {"fog_mode": "exponential", "density": 0.5, "depth_begin": 10.0, "depth_end": 90.0, "depth_curve": 0.5,
                                                          "aerial_perspective": 0.25, "sun_scatter": 0.125, "light_color": (0.1, 0.2, 0.3),
                                                          "sun_color": (0.9, 0.8, 0.7), "sun_direction": (0.0, 0.8, 0.6), "sky_color": (0.4, 0.5, 0.6)}, False),
    "present_options": (_lib.ow_present_options, {"downsample": 2, "tonemap": "reinhard", "exposure": 1.5, "white": 2.0, "srgb": 0, "brightness": 0.9,
                                                  "contrast": 1.1, "saturation": 1.2}, False),
    "radiance_options": (_lib.ow_radiance_options, {"levels": 4, "samples": 32, "base_width": 256}, False),
    "sky_light_options": (_lib.ow_radiance_light_options, {"ambient_energy": 0.5, "reflection_energy": 0.75, "specular": 0.25}, False),
    "shadow_frame": (_lib.ow_shadow_frame, {"light_direction": (0.0, -0.8, 0.6), "half_extent": 50.0, "center": (1.0, 2.0, 3.0), "depth_range": 80.0,
                                            "cast_both_sides": True, "lane_box": 10}, False),
    "shadow_options": (_lib.ow_shadow_options, {"bias": 0.5, "normal_bias": 3.0, "opacity": 0.5, "filter_taps": 3, "receive_water": True}, False),
}
# further inputs: falsy flags, an enumeration by number and by an unknown word, a falloff centre of None
MORE = {
    "query_options": [{"falloff_center": None}, {"max_iterations": 7.9}],
    "buoyancy_options": [{"warm_start": False, "water_velocity": 0}, {"warm_start": True}, {"water_velocity": True}],
    "raycast_options": [{"query_tolerance": 0.003}, {"max_iterations": 9}, {"tolerance": 0.004}],
    "render_options": [{"falloff": False}, {"falloff": True, "falloff_center": (1.0, 2.0)}, {"falloff_center": (1.0, 2.0)}, {"falloff": True, "falloff_center": None},
                       {"roughness": 0.5}, {"max_samples": 5}],
    "mesh_options": [{"falloff": False}, {"cull_back": False}, {"falloff": True, "falloff_center": None}, {"falloff_center": None}, {"falloff_center": (1.0, 2.0)}],
    "solid_options": [{"two_sided": False}],
    "environment_options": [{"fog_mode": 0}, {"fog_mode": "depth"}, {"fog_mode": "mist"}],
    "present_options": [{"tonemap": 0}, {"tonemap": "linear"}, {"tonemap": "filmic"}, {"tonemap": "aces"}],
    "shadow_frame": [{"cast_both_sides": False}],
    "shadow_options": [{"receive_water": False}],
    "spray_options": [{"particle_scale": (1.0, 2.0)}],
}


def converter_cases(name):
    """[label, input, camera or None] of one converter"""
    _, keys, takes_camera = CONVERTERS[name]
    cases = [["None", None], ["{}", {}]] + [[k, {k: v}] for k, v in keys.items()] + [["all", dict(keys)]]
    cases += [["unknown", {"bogus": 1}], ["unknown two", {"zeta": 1, "alpha": 2}], ["unknown among known", dict(keys, zeta=1, alpha=2)]]
    cases += [[json.dumps(m, sort_keys=True), m] for m in MORE.get(name, [])]
    out = []
    for label, value in cases:
        for c in ((None, cam()) if takes_camera else (None,)):
            out.append([label + (" +camera" if c is not None else ""), value, c])
    return out


def options():
    out = {}
    for name, (struct, _, takes_camera) in CONVERTERS.items():
        fn = getattr(W, name)
        rec = {label: attempt(fn, *((value, c) if takes_camera else (value,))) for label, value, c in converter_cases(name)}
        given = struct()
        rec["a struct comes back itself"] = fn(given) is given
        out[name] = rec
    c = cam(8, 6)
    out["present_size"] = {label: attempt(W.present_size, c, o) for label, o in (("None", None), ("{}", {}), ("downsample 2", {"downsample": 2}),
                                                                                  ("downsample 0", {"downsample": 0}), ("downsample 4", {"downsample": 4}),
                                                                                  ("unknown", {"bogus": 1}))}
    given = _lib.ow_present_options(downsample=3)
    out["present_size"]["struct"] = attempt(W.present_size, c, given)
    out["camera"] = {"level": attempt(W.camera, (1.0, 2.0, 3.0), np.eye(3), 60.0, 640, 360, 4000.0),
                     "nine values": attempt(W.camera, [1, 2, 3], list(range(9)), 45, 7.0, 5.0, 10),
                     "short basis": attempt(W.camera, (1.0, 2.0, 3.0), np.eye(2), 60.0, 4, 4, 10.0)}
    out["rays"] = {"scalar distance": attempt(W.rays, [[0, 1, 2], [3, 4, 5]], [[0, -1, 0], [1, -2, 3]], 50.0),
                   "distances": attempt(W.rays, [0, 1, 2, 3, 4, 5], [0, -1, 0, 1, -2, 3], [5.0, 6.0]),
                   "mismatch": attempt(W.rays, [[0, 1, 2]], [[0, -1, 0], [1, -2, 3]], 50.0)}
    out["box_hull"] = {"2x1x3": attempt(W.box_hull, (2.0, 1.0, 3.0), (2, 1, 3)),
                       "body and centre": attempt(W.box_hull, (1.0, 2.0, 4.0), (1, 2, 2), body=3, center=(0.5, -0.25, 1.0))}
    out["box_mass_properties"] = {"box": attempt(W.box_mass_properties, (2.0, 1.0, 3.0), 500.0), "ints": attempt(W.box_mass_properties, (1, 2, 3), 2)}
    out["clipmap_origin"] = {"positive": attempt(W.clipmap_origin, (10.5, 3.0, 33.0), 16.0), "negative": attempt(W.clipmap_origin, (-10.5, 3.0, -0.25), 16.0),
                             "on the grid": attempt(W.clipmap_origin, (32.0, 0.0, -16.0), 16)}
    out["JONSWAP"] = [attempt(W.JONSWAP_alpha), attempt(W.JONSWAP_peak_angular_frequency), attempt(W.JONSWAP_alpha, 10.0, 100e3)]
    return out


# ---- 3. the call traces ----------------------------------------------------------------------------------------------------------------------
class FakeBuffer:
    """what the wrapper reads of a torch tensor: `nbytes` bytes of uint8 at `address`"""

    def __init__(self, nbytes, address):
        self.nbytes, self.address = nbytes, address

    def data_ptr(self):
        return self.address

    def numel(self):
        return self.nbytes

    def element_size(self):
        return 1


class FloatBuffer(FakeBuffer):
    """a float32 tensor of `nbytes` / 4 elements"""

    def numel(self):
        return self.nbytes // 4

    def element_size(self):
        return 4


def argument(a, kind):
    """integers and floats keep their value, byref(struct) and a struct or an array of structs are their bytes, None stays, anything else is
    "ptr".  So is an address that differs from run to run: an integer where the entry point (`kind`: its argtype) takes a pointer, unless it
    lies below 64 KiB, where nothing is ever mapped -- those are this script's fake handles and device addresses, and they keep their value"""
    if a is None or isinstance(a, (bool, float)):
        return a
    if isinstance(a, int):
        pointer = kind is C.c_void_p or issubclass(kind, C._Pointer)
        return a if not pointer or 0 <= a < 0x10000 else "ptr"
    inner = getattr(a, "_obj", a)
    if isinstance(inner, C.Structure) or (isinstance(inner, C.Array) and issubclass(inner._type_, C.Structure)):
        return {"bytes": bytes(inner).hex()}
    return "ptr"


class StubLibrary:
    """every ow_* entry point records [name, arguments] and answers OW_OK, or what `answers` holds for it; the *_default entry points and the
    JONSWAP statics are the real library's"""

    def __init__(self, answers=None):
        self.calls, self.answers, self.real = [], dict(answers or {}), REAL

    def __getattr__(self, name):
        if not name.startswith("ow_"):
            raise AttributeError(name)
        if name.endswith("_default") or name.startswith("ow_jonswap"):
            return getattr(self.real, name)
        if name not in _lib.SIGNATURES:
            raise AttributeError(name)

        def entry(*args):
            self.calls.append([name] + [argument(a, kind) for a, kind in zip(args, _lib.SIGNATURES[name][1])])
            return self.answers.get(name, _lib.OW_OK)
        return entry

    def take(self):
        calls, self.calls = self.calls, []
        return calls


REAL = None
CONTEXT, GROUP = 0xC0DE, 0x6A0B
SCALES = [[0.02, 0.02, 1.0, 1.0], [0.05, 0.05, 0.5, 0.25]]
ANSWERS = {"ow_last_kernel_family": 3, "ow_last_batch_cascades": 2, "ow_tick_group_depth": 4, "ow_cascades_remaining": 0, "ow_group_context": 0x5AAD,
           "ow_group_num_cascades": 6, "ow_group_cascades_remaining": 0}
# not traced, each with its reason
EXCLUDED = {"readback_wait": "its return value is a view of memory the library hands back, which the stand-in library does not have"}


def traced(stub, fn, *a, **kw):
    result = attempt(fn, *a, **kw)
    return {"calls": stub.take(), "result": summary(result)}


def summary(v):
    """of a result, what does not depend on what the library would have written: an array's dtype and shape"""
    if isinstance(v, dict) and "shape" in v and "bytes" in v:
        return {"dtype": v["dtype"], "shape": v["shape"]}
    if isinstance(v, dict):
        return {k: summary(x) for k, x in v.items()}
    if isinstance(v, list):
        return [summary(x) for x in v]
    return v


def generator(stub, **attrs):
    gen = W()
    gen.map_size, gen.num_cascades, gen._lib, gen.context = 8, 2, stub, CONTEXT
    for k, v in attrs.items():
        setattr(gen, k, v)
    gen.free = lambda: None
    return gen


INIT_FLAGS = [{}, {"debug_f32": True}, {"tick_groups": False}, {"run_as_calls": True}, {"run_as_reference": True}, {"always_regenerate_spectrum": True},
              {"lazy_scratch": True}, {"single_stream": True}, {"bodies_kernels": "fused"}, {"bodies_kernels": "split"}, {"bodies_kernels": "both"},
              {"kernels": "standard"}, {"kernels": "layer_parallel"}, {"kernels": "compact"}, {"kernels": "layer_parallel_compact"}, {"kernels": "fast"},
              {"group_forms": ("lp", None)}, {"group_forms": ("compact", "plain")}, {"group_forms": (None, "pipe")}, {"group_forms": ("wide", None)},
              {"group_forms": (None, "deep")}, {"device_id": 3, "stream": 0x5712, "external_maps": (0xD15B, 0x2022), "depth": 35.5},
              {"debug_f32": True, "tick_groups": False, "run_as_calls": True, "run_as_reference": True, "always_regenerate_spectrum": True, "lazy_scratch": True,
               "single_stream": True, "bodies_kernels": "fused", "kernels": "layer_parallel_compact", "group_forms": ("compact", "pipe")}]


def traces():
    """{label: {"calls": [[entry point, argument ...] ...], "result": ...}} of every wrapper method on the stand-in library"""
    stub = StubLibrary(ANSWERS)
    load, _lib.load = _lib.load, lambda: stub     # init_gpu and the un-initialised update() load the library themselves
    try:
        return _traces(stub)
    finally:
        _lib.load = load


def _traces(stub):
    out = {}
    t = lambda label, fn, *a, **kw: out.__setitem__(label, traced(stub, fn, *a, **kw))   # noqa: E731

    # init_gpu, attribute by attribute
    for attrs in INIT_FLAGS:
        gen = W()
        gen.map_size = 16
        for k, v in attrs.items():
            setattr(gen, k, v)
        t("init_gpu " + json.dumps(attrs, sort_keys=True), gen.init_gpu, 3)
        gen.context = None
    gen = W()
    gen.map_size = 16
    gen.init_gpu(2)
    t("init_gpu twice", gen.init_gpu, 4)
    t("free", gen.free)
    t("free twice", gen.free)
    stub.take()

    # the scheduler calls
    gen = generator(stub)
    params = [WaveCascadeParameters(tile_length=(88.0, 88.0), spectrum_seed=(1, 2)), WaveCascadeParameters(wind_speed=5.0, whitecap=0.25)]
    t("update", gen.update, 1 / 60, params)
    t("_process", gen._process)
    t("update_all", gen.update_all, 1 / 60, params)
    t("run", gen.run, 1 / 60, params, 5)
    t("pass_num_cascades_remaining", lambda: gen.pass_num_cascades_remaining)
    fresh = W()
    fresh.map_size = 8
    t("update without init_gpu", fresh.update, 0.5, params[:1])
    fresh.context = None
    t("sync", gen.sync)
    t("debug_inject_fault", gen.debug_inject_fault, 5)
    t("get_maps", gen.get_maps, 1)
    t("set_normal_map", gen.set_normal_map, 1, np.zeros((8, 8, 4), np.float16))
    t("readback_begin", gen.readback_begin, [0, 2])

    # points: samples, queries, velocity, buoyancy, ray casts, views
    xz = [[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]
    q = {"max_iterations": 5, "falloff_center": (1.0, 2.0)}
    t("sample_surface", gen.sample_surface, xz, SCALES)
    for label, o in (("", None), (" options", q), (" struct", W.query_options(q)), (" unknown", {"bogus": 1})):
        t("query_surface" + label, gen.query_surface, xz, SCALES, o)
        t("query_velocity" + label, gen.query_velocity, xz, SCALES, o)
    xzd, outd = FloatBuffer(3 * 8, 0x1000), FakeBuffer(3 * 128, 0x2000)
    t("query_surface_async", gen.query_surface_async, xzd, SCALES, outd)
    t("query_surface_async options count", gen.query_surface_async, 0x1000, SCALES, 0x2000, q, 2)
    t("query_surface_async raw address", gen.query_surface_async, 0x1000, SCALES, 0x2000)
    t("query_surface_async short", gen.query_surface_async, xzd, SCALES, FakeBuffer(3 * 128 - 1, 0x2000))
    t("query_velocity_async", gen.query_velocity_async, xzd, SCALES, FakeBuffer(3 * 32, 0x2000))
    t("query_velocity_async options count", gen.query_velocity_async, 0x1000, SCALES, 0x2000, q, 2)
    t("query_velocity_async raw address", gen.query_velocity_async, 0x1000, SCALES, 0x2000)
    t("query_velocity_async short", gen.query_velocity_async, xzd, SCALES, FakeBuffer(3 * 32 - 1, 0x2000))
    t("update_velocity", gen.update_velocity)
    t("update_velocity some", gen.update_velocity, [1])
    t("velocity_ptrs", gen.velocity_ptrs)
    t("velocity_map", gen.velocity_map, 1)
    t("velocity_stats", gen.velocity_stats)

    hull = W.box_hull((2.0, 1.0, 2.0), (2, 1, 2))
    bodies = np.zeros(2, W.BUOYANCY_BODY)
    bodies["point_count"] = [3, 1]
    b = {"density": 1000.0, "warm_start": True, "max_iterations": 3}
    pts = np.zeros(len(hull), W.BUOYANCY_POINT)
    t("buoyancy", gen.buoyancy, bodies, hull, SCALES)
    t("buoyancy options points", gen.buoyancy, bodies, hull, SCALES, b, pts)
    t("buoyancy short points", gen.buoyancy, bodies, hull, SCALES, None, pts[:2])
    t("buoyancy wrong points", gen.buoyancy, bodies, hull, SCALES, None, np.zeros(len(hull), W.HULL_POINT))
    t("buoyancy unknown", gen.buoyancy, bodies, hull, SCALES, {"bogus": 1})
    bd, hd, rd, pd = FakeBuffer(2 * 96, 0x3000), FakeBuffer(4 * 32, 0x4000), FakeBuffer(2 * 64, 0x5000), FakeBuffer(4 * 64, 0x6000)
    t("buoyancy_async", gen.buoyancy_async, bd, hd, SCALES, rd, pd)
    t("buoyancy_async options counts", gen.buoyancy_async, 0x3000, 0x4000, SCALES, 0x5000, 0x6000, b, 1, 3)
    t("buoyancy_async raw bodies", gen.buoyancy_async, 0x3000, hd, SCALES, rd, pd)
    t("buoyancy_async raw hull", gen.buoyancy_async, bd, 0x4000, SCALES, rd, pd)
    t("buoyancy_async short results", gen.buoyancy_async, bd, hd, SCALES, FakeBuffer(2 * 64 - 1, 0x5000), pd)

    rays = W.rays([[0, 5, 0], [1, 5, 1]], [[0, -1, 0], [0, -1, 0.5]], 20.0)
    r = {"max_samples": 64, "query_tolerance": 0.01}
    for label, o in (("", None), (" options", r), (" struct", W.raycast_options(r)), (" unknown", {"bogus": 1})):
        t("raycast_surface" + label, gen.raycast_surface, rays, SCALES, o)
    t("raycast_surface_async", gen.raycast_surface_async, FakeBuffer(2 * 32, 0x7000), SCALES, FakeBuffer(2 * 192, 0x8000))
    t("raycast_surface_async options count", gen.raycast_surface_async, 0x7000, SCALES, 0x8000, r, 1)
    t("raycast_surface_async raw address", gen.raycast_surface_async, 0x7000, SCALES, 0x8000)
    t("raycast_surface_async short", gen.raycast_surface_async, FakeBuffer(2 * 32, 0x7000), SCALES, FakeBuffer(2 * 192 - 1, 0x8000))

    c = cam()
    npix = c.width * c.height
    rgbad, pixd = FakeBuffer(npix * 4, 0x9000), FakeBuffer(npix * 128, 0xA000)
    rec = np.zeros((c.height, c.width), W.RENDER_PIXEL)
    rec["t"] = 3.0
    v = {"roughness": 0.5, "falloff": True, "max_samples": 16}
    t("render_view", gen.render_view, c, SCALES)
    t("render_view options no pixels", gen.render_view, c, SCALES, v, False)
    t("render_view unknown", gen.render_view, c, SCALES, {"bogus": 1})
    t("render_view_async", gen.render_view_async, c, SCALES, rgbad)
    t("render_view_async pixels options", gen.render_view_async, c, SCALES, None, pixd, v)
    t("render_view_async short", gen.render_view_async, c, SCALES, FakeBuffer(npix * 4 - 1, 0x9000))

    # bodies
    state = np.zeros(2, W.RIGID_BODY)
    t("bodies_create", gen.bodies_create, state, hull)
    bs = wg._BodySet(0xB0D1, 5, 9)
    t("bodies_step", gen.bodies_step, bs, SCALES, 4, 1 / 240)
    t("bodies_step options", gen.bodies_step, bs, SCALES, 4, 1 / 240, b)
    t("bodies_step struct", gen.bodies_step, bs, SCALES, 2, 0.01, W.bodies_options(b))
    t("bodies_step unknown", gen.bodies_step, bs, SCALES, 4, 1 / 240, {"bogus": 1})
    t("bodies_state", gen.bodies_state, bs)
    t("bodies_state first", gen.bodies_state, bs, 2)
    t("bodies_state first count", gen.bodies_state, bs, 1, 2)
    t("bodies_set_state", gen.bodies_set_state, bs, state, 1)
    t("bodies_results", gen.bodies_results, bs)
    t("bodies_results first count", gen.bodies_results, bs, 3, 1)
    t("bodies_device_ptrs", gen.bodies_device_ptrs, bs)
    t("bodies_stats", gen.bodies_stats, bs)
    t("bodies_stats not faulted", gen.bodies_stats, bs, False)
    t("sync_stats", gen.sync_stats)

    # mesh
    verts, tris = [[0, 0, 0], [1, 0, 0], [0, 0, 1], [1, 0, 1]], [[0, 1, 2], [2, 1, 3]]
    m = {"near": 0.1, "cull_back": True, "falloff": True, "roughness": 0.25}
    t("mesh_create", gen.mesh_create, verts, tris)
    mesh = wg._Mesh(0x3E5A, 4, 2)
    t("mesh_displace", gen.mesh_displace, mesh, (16.0, 0.0, 32.0), SCALES)
    t("mesh_displace options camera", gen.mesh_displace, mesh, (16.0, 0.0, 32.0), SCALES, m, c)
    t("mesh_displace falloff without camera", gen.mesh_displace, mesh, (16.0, 0.0, 32.0), SCALES, m)
    t("mesh_device_ptrs", gen.mesh_device_ptrs, mesh)
    t("mesh_draw", gen.mesh_draw, mesh, c, (0.0, 0.0, 0.0), SCALES)
    t("mesh_draw options no pixels", gen.mesh_draw, mesh, c, (0.0, 0.0, 0.0), SCALES, m, False)
    t("mesh_draw unknown", gen.mesh_draw, mesh, c, (0.0, 0.0, 0.0), SCALES, {"bogus": 1})
    t("mesh_draw_async", gen.mesh_draw_async, mesh, c, (0.0, 0.0, 0.0), SCALES, rgbad)
    t("mesh_draw_async pixels options", gen.mesh_draw_async, mesh, c, (0.0, 0.0, 0.0), SCALES, None, pixd, m)
    t("mesh_draw_async short", gen.mesh_draw_async, mesh, c, (0.0, 0.0, 0.0), SCALES, rgbad, FakeBuffer(npix * 128 - 1, 0xA000))
    t("mesh_stats", gen.mesh_stats, mesh)

    # spray and billboards
    s = {"amount": 32, "random_seed": 9}
    t("spray_create", gen.spray_create)
    t("spray_create options", gen.spray_create, s)
    t("spray_create struct", gen.spray_create, W.spray_options(s))
    t("spray_create unknown", gen.spray_create, {"bogus": 1})
    spray = wg._Spray(0x5B4A, 8)
    t("spray_step", gen.spray_step, spray, 1 / 60, SCALES)
    t("spray_read", gen.spray_read, spray)
    t("spray_live_count", gen.spray_live_count, spray)
    t("spray_device_ptrs", gen.spray_device_ptrs, spray)
    t("spray_stats", gen.spray_stats, spray)
    tex, tex2 = np.zeros((2, 3, 4), np.uint8), np.zeros((5, 4, 4), np.uint8)
    t("spray_material_create", gen.spray_material_create, tex, tex2)
    t("spray_material_create options", gen.spray_material_create, tex, tex2, {"max_alpha": 0.5})
    t("spray_material_create flat texture", gen.spray_material_create, tex, np.zeros((5, 4), np.uint8))
    t("spray_material_create unknown", gen.spray_material_create, tex, tex2, {"bogus": 1})
    mat = wg._SprayMaterial(0x3A7E)
    d = {"near": 0.2, "bin_side": 8}
    inst = np.zeros(3, W.SPRAY_INSTANCE)
    t("spray_draw", gen.spray_draw, spray, mat, c)
    t("spray_draw options pixels", gen.spray_draw, spray, mat, c, d, rec)
    t("spray_draw pixels no rgba", gen.spray_draw, spray, mat, c, None, rec, False)
    t("spray_draw wrong pixels", gen.spray_draw, spray, mat, c, None, rec.T)
    t("spray_draw unknown", gen.spray_draw, spray, mat, c, {"bogus": 1})
    t("spray_draw_instances", gen.spray_draw_instances, mat, inst, 1.5, c)
    t("spray_draw_instances none options pixels", gen.spray_draw_instances, mat, inst[:0], 1.5, c, d, rec, False)
    t("spray_draw_async", gen.spray_draw_async, spray, mat, c, rgbad)
    t("spray_draw_async pixels options", gen.spray_draw_async, spray, mat, c, rgbad, pixd, d)
    t("spray_draw_async short", gen.spray_draw_async, spray, mat, c, FakeBuffer(npix * 4 - 1, 0x9000))
    t("spray_draw_stats", gen.spray_draw_stats)
    t("spray_draw_stats no counters", gen.spray_draw_stats, False)

    # solids and shadows
    so = {"color": (1.0, 0.0, 0.0), "two_sided": True}
    t("solid_create", gen.solid_create, verts, tris)
    solid = wg._Solid(0x5011, 4, 2)
    tf = np.zeros((2, 12), np.float32)
    t("solid_draw", gen.solid_draw, solid, bs, c)
    t("solid_draw options pixels range", gen.solid_draw, solid, bs, c, so, rec, False, 1, 3)
    t("solid_draw first", gen.solid_draw, solid, bs, c, first=2)
    t("solid_draw unknown", gen.solid_draw, solid, bs, c, {"bogus": 1})
    t("solid_draw_instances", gen.solid_draw_instances, solid, tf, c)
    t("solid_draw_instances none options pixels", gen.solid_draw_instances, solid, tf[:0], c, so, rec, False)
    t("solid_draw_async", gen.solid_draw_async, solid, bs, c, rgbad)
    t("solid_draw_async pixels options range", gen.solid_draw_async, solid, bs, c, rgbad, pixd, so, 1, 2)
    t("solid_draw_async first", gen.solid_draw_async, solid, bs, c, rgbad, first=4)
    t("solid_draw_async short", gen.solid_draw_async, solid, bs, c, rgbad, FakeBuffer(npix * 128 - 1, 0xA000))
    t("solid_draw_stats", gen.solid_draw_stats)
    t("solid_draw_stats no counters", gen.solid_draw_stats, False)
    t("shadow_map_create", gen.shadow_map_create, 64)
    sm = wg.ShadowMap(0x5AD0, 16)
    sh = {"opacity": 0.5, "receive_water": True}
    t("shadow_map_begin", gen.shadow_map_begin, sm)
    t("shadow_map_begin frame", gen.shadow_map_begin, sm, {"half_extent": 20.0, "cast_both_sides": True})
    t("shadow_map_begin struct", gen.shadow_map_begin, sm, W.shadow_frame({"lane_box": 4}))
    t("shadow_map_begin unknown", gen.shadow_map_begin, sm, {"bogus": 1})
    t("shadow_map_cast", gen.shadow_map_cast, sm, solid, bs)
    t("shadow_map_cast range", gen.shadow_map_cast, sm, solid, bs, 1, 2)
    t("shadow_map_cast first", gen.shadow_map_cast, sm, solid, bs, 3)
    t("shadow_map_cast_instances", gen.shadow_map_cast_instances, sm, solid, tf)
    t("shadow_map_cast_instances none", gen.shadow_map_cast_instances, sm, solid, tf[:0])
    t("shadow_map_read", gen.shadow_map_read, sm)
    t("shadow_apply", gen.shadow_apply, sm, c, rec)
    t("shadow_apply options rgba", gen.shadow_apply, sm, c, rec, sh, True)
    t("shadow_apply no map", gen.shadow_apply, None, c, rec)
    t("shadow_apply unknown", gen.shadow_apply, sm, c, rec, {"bogus": 1})
    t("shadow_apply_async", gen.shadow_apply_async, sm, c, pixd)
    t("shadow_apply_async rgba options", gen.shadow_apply_async, None, c, pixd, rgbad, sh)
    t("shadow_apply_async short", gen.shadow_apply_async, sm, c, FakeBuffer(npix * 128 - 1, 0xA000))
    t("shadow_stats", gen.shadow_stats, sm)
    t("shadow_stats no counters", gen.shadow_stats, sm, False)

    # sky, environment, present, radiance
    pano = np.zeros((4, 8, 4), np.uint8)
    t("sky_create", gen.sky_create, pano)
    t("sky_create options", gen.sky_create, pano, {"energy": 2.0})
    t("sky_create flat", gen.sky_create, pano[..., 0])
    t("sky_create unknown", gen.sky_create, pano, {"bogus": 1})
    sky = wg.Sky(0x5C1, 8, 4)
    e, p, ro, sl = {"fog_mode": "exponential", "density": 0.1}, {"downsample": 2, "tonemap": "linear"}, {"levels": 3}, {"specular": 0.25}
    t("environment_apply", gen.environment_apply, c, rec)
    t("environment_apply sky options", gen.environment_apply, c, rec, sky, e)
    t("environment_apply unknown", gen.environment_apply, c, rec, None, {"bogus": 1})
    t("environment_apply_async", gen.environment_apply_async, c, pixd)
    t("environment_apply_async sky options", gen.environment_apply_async, c, pixd, sky, e)
    t("environment_apply_async short", gen.environment_apply_async, c, FakeBuffer(npix * 128 - 1, 0xA000))
    t("present", gen.present, c, rec)
    t("present options linear", gen.present, c, rec, p, True)
    t("present unknown", gen.present, c, rec, {"bogus": 1})
    t("present_async", gen.present_async, c, pixd, rgbad)
    t("present_async linear options", gen.present_async, c, pixd, None, FakeBuffer(npix * 4, 0xB000), p)
    t("present_async short pixels", gen.present_async, c, FakeBuffer(npix * 128 - 1, 0xA000), rgbad)
    t("present_async short rgba", gen.present_async, c, pixd, FakeBuffer(npix * 4 - 1, 0x9000))
    t("present_async short linear", gen.present_async, c, pixd, rgbad, FakeBuffer(npix * 16 - 1, 0xB000))
    t("radiance_create", gen.radiance_create, sky)
    t("radiance_create options", gen.radiance_create, sky, ro)
    t("radiance_create unknown", gen.radiance_create, sky, {"bogus": 1})
    rad = wg.Radiance(0x4AD, 6)
    t("radiance_level", gen.radiance_level, rad, 2)
    t("radiance_level irradiance", gen.radiance_level, rad, "irradiance")
    t("sky_light_apply", gen.sky_light_apply, rad, c, rec)
    t("sky_light_apply none options", gen.sky_light_apply, None, c, rec, sl)
    t("sky_light_apply unknown", gen.sky_light_apply, rad, c, rec, {"bogus": 1})
    t("sky_light_apply_async", gen.sky_light_apply_async, rad, c, pixd)
    t("sky_light_apply_async none options", gen.sky_light_apply_async, None, c, pixd, sl)
    t("sky_light_apply_async short", gen.sky_light_apply_async, rad, c, FakeBuffer(npix * 128 - 1, 0xA000))

    # every destroy: the handle is spent, a second destroy does nothing
    for name, obj in (("bodies_destroy", bs), ("mesh_destroy", mesh), ("spray_destroy", spray), ("spray_material_destroy", mat), ("solid_destroy", solid),
                      ("sky_destroy", sky), ("radiance_destroy", rad), ("shadow_map_destroy", sm)):
        t(name, getattr(gen, name), obj)
        t(name + " twice", getattr(gen, name), obj)
        out[name + " twice"]["handle"] = show(obj.handle)

    # the debug and measurement surface
    t("get_push_constants", gen.get_push_constants, 1)
    t("get_maps_f32", gen.get_maps_f32, 1)
    t("get_spectrum", gen.get_spectrum, 1)
    t("debug_set_spectrum", gen.debug_set_spectrum, 1, np.zeros((8, 8), np.complex64))
    t("debug_set_spectrum omega", gen.debug_set_spectrum, 1, np.zeros((8, 8), np.complex64), np.zeros((8, 8), np.float32))
    t("debug_set_spectrum wrong h0", gen.debug_set_spectrum, 1, np.zeros((8, 4), np.complex64))
    t("debug_set_spectrum wrong omega", gen.debug_set_spectrum, 1, np.zeros((8, 8), np.complex64), np.zeros((4, 8), np.float32))
    t("get_intermediate", gen.get_intermediate, 1)
    for name in ("last_kernel_family", "last_batch_cascades", "tick_group_depth", "lookahead_stats", "chain_stats", "spectrum_stats", "timing_read_launches",
                 "timing_read", "probe_kernel_times"):
        t(name, getattr(gen, name))
    t("timing_read_launches keep", gen.timing_read_launches, False)
    t("timing_read keep", gen.timing_read, False)
    t("probe_kernel_times reps", gen.probe_kernel_times, 7)
    for enable in (False, True, 1, 2, 3):
        t(f"timing {enable!r}", gen.timing, enable)

    # the group
    for attrs in ({}, {"debug_f32": True}, {"tick_groups": False}, {"force_peer_path": True}, {"depth": 12.5}):
        grp = WaveGeneratorGroup()
        grp.map_size = 16
        for k, v in attrs.items():
            setattr(grp, k, v)
        t("group init_gpu " + json.dumps(attrs, sort_keys=True), grp.init_gpu, [2, 0, 1], 2, 1)
        grp.group = None
    t("group init_gpu no devices", grp.init_gpu, [], 2)
    grp = WaveGeneratorGroup()
    grp.map_size, grp._lib, grp.group, grp.num_devices, grp.cascades_per_device = 8, stub, GROUP, 2, 3
    t("group num_cascades", lambda: grp.num_cascades)
    t("group pass_num_cascades_remaining", lambda: grp.pass_num_cascades_remaining)
    t("group update", grp.update, 1 / 60, params)
    t("group _process", grp._process)
    t("group update_all", grp.update_all, 1 / 60, params)
    t("group run", grp.run, 1 / 60, params, 3)
    for name in ("sync", "gather_begin", "gather_wait", "gather_stats", "link_info", "device_ptrs"):
        t("group " + name, getattr(grp, name))
    t("group get_maps", grp.get_maps, 4)
    t("group sample_surface", grp.sample_surface, xz, SCALES)
    t("group query_surface", grp.query_surface, xz, SCALES)
    t("group query_surface options", grp.query_surface, xz, SCALES, q)
    t("group query_surface unknown", grp.query_surface, xz, SCALES, {"bogus": 1})
    t("group buoyancy", grp.buoyancy, bodies, hull, SCALES)
    t("group buoyancy options points", grp.buoyancy, bodies, hull, SCALES, b, pts)
    t("group buoyancy short points", grp.buoyancy, bodies, hull, SCALES, None, pts[:2])
    t("group raycast_surface", grp.raycast_surface, rays, SCALES)
    t("group raycast_surface options", grp.raycast_surface, rays, SCALES, r)
    view = grp.shard(1)
    t("group shard", lambda: [view.map_size, view.context.value, view.num_cascades, view._lib is stub, view.free()])
    t("group shard get_maps", view.get_maps, 0)
    t("group shard last_kernel_family", view.last_kernel_family)
    t("group free", grp.free)
    t("group free twice", grp.free)
    return out


def record(recorded_from):
    global REAL
    REAL = _lib.load()
    return plain({"recorded_from": recorded_from, "excluded": EXCLUDED, "surface": surface(), "options": options(), "traces": traces()})

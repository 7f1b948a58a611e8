"""Host-side mirror of the reference's generator interface on top of the C-ABI.

`WaveCascadeParameters` mirrors assets/water/wave_cascade_parameters.gd (same field names, defaults,
clamps and dirty-flag setters); `WaveGenerator` mirrors assets/water/wave_generator.gd (map_size,
init_gpu, update, _process, descriptors, JONSWAP statics).  All compute happens in
libocean_waves.so (HIP, gfx950); this file holds no numerics beyond packing the parameter record.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import (OW_FLAG_ALWAYS_REGENERATE_SPECTRUM, OW_FLAG_LAZY_SCRATCH, OW_FLAG_SINGLE_STREAM, OW_FLAG_DEBUG_F32, OW_FLAG_GROUP_P1_COMPACT, OW_FLAG_GROUP_P1_LP, OW_FLAG_GROUP_P2_PIPE, OW_FLAG_GROUP_P2_PLAIN, OW_FLAG_KERNELS_COMPACT,
                   OW_FLAG_KERNELS_LAYER_PARALLEL, OW_FLAG_KERNELS_STANDARD, OW_FLAG_NO_TICK_GROUPS, OW_FLAG_RUN_AS_CALLS, OW_FLAG_RUN_AS_REFERENCE_SCHEDULE,
                   ow_cascade_params, ow_config)

G = 9.81       # wave_generator.gd:5
DEPTH = 20.0   # wave_generator.gd:6


def _scales(map_scales):
    """map_scales [C][4] (water.gd:105-109) as the contiguous float32 array the C-ABI reads; len() is num_cascades"""
    return np.ascontiguousarray(map_scales, np.float32).reshape(-1, 4)


def _addr(buf, optional=False):
    """the device address of anything with a data_ptr() (a torch tensor) or of an integer address; optional: None passes (an output a
    picture call is not asked for)"""
    if buf is None and optional:
        return None
    return int(buf.data_ptr()) if hasattr(buf, "data_ptr") else int(buf)


def _ref(o):
    """an optional struct argument: NULL for None"""
    return C.byref(o) if o is not None else None


def _check_device_size(buf, count, size, name="out_device", unit="records"):
    """ValueError for a device buffer that knows its size and holds fewer than `count` units of `size` bytes; a bare address passes"""
    if hasattr(buf, "numel") and hasattr(buf, "element_size") and buf.numel() * buf.element_size() < count * size:
        raise ValueError(f"{name} holds fewer than {count} {unit} of {size} bytes")


def _dirty(name, clamp=None):
    """@export var with `set(value): ...; should_generate_spectrum = true` (wave_cascade_parameters.gd:7-35)"""
    attr = "_" + name

    def getter(self):
        return getattr(self, attr)

    def setter(self, value):
        setattr(self, attr, clamp(value) if clamp else value)
        self.should_generate_spectrum = True

    return property(getter, setter)


class WaveCascadeParameters:
    """wave_cascade_parameters.gd:1-56 (the imgui mirror fields :44-56 are UI-only and omitted)."""
    tile_length = _dirty("tile_length", lambda v: (float(v[0]), float(v[1])))                 # :7
    wind_speed = _dirty("wind_speed", lambda v: max(0.0001, float(v)))                        # :15
    wind_direction = _dirty("wind_direction", float)                                          # :17
    fetch_length = _dirty("fetch_length", lambda v: max(0.0001, float(v)))                    # :20
    swell = _dirty("swell", float)                                                            # :22
    spread = _dirty("spread", float)                                                          # :25
    detail = _dirty("detail", float)                                                          # :28
    whitecap = _dirty("whitecap", float)      # yes, the reference re-generates on these too    :32-35
    foam_amount = _dirty("foam_amount", float)

    def __init__(self, **kw):
        self.displacement_scale = 1.0   # :9  (consumer-side only; no dirty flag)
        self.normal_scale = 1.0         # :11
        self.tile_length = (50.0, 50.0)
        self.wind_speed = 20.0
        self.wind_direction = 0.0
        self.fetch_length = 550.0
        self.swell = 0.8
        self.spread = 0.2
        self.detail = 1.0
        self.whitecap = 0.5
        self.foam_amount = 5.0
        self.spectrum_seed = (0, 0)            # :37 Vector2i.ZERO
        self.should_generate_spectrum = True   # :38
        self.time = 0.0                        # :40
        self.foam_grow_rate = 0.0              # :41
        self.foam_decay_rate = 0.0             # :42
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(f"WaveCascadeParameters has no field {k!r}")
            setattr(self, k, v)

    def _pack(self, c):
        c.tile_length[0], c.tile_length[1] = self.tile_length
        c.displacement_scale, c.normal_scale = self.displacement_scale, self.normal_scale
        c.wind_speed, c.wind_direction, c.fetch_length = self.wind_speed, self.wind_direction, self.fetch_length
        c.swell, c.spread, c.detail = self.swell, self.spread, self.detail
        c.whitecap, c.foam_amount = self.whitecap, self.foam_amount
        c.spectrum_seed[0], c.spectrum_seed[1] = int(self.spectrum_seed[0]), int(self.spectrum_seed[1])
        c.should_generate_spectrum = 1 if self.should_generate_spectrum else 0
        c.time, c.foam_grow_rate, c.foam_decay_rate = self.time, self.foam_grow_rate, self.foam_decay_rate


class _Descriptor:
    """stand-in for RenderingContext.Descriptor (render_context.gd:23-28): `.rid` is the device pointer"""

    def __init__(self, rid, layer_stride):
        self.rid, self.layer_stride = rid, layer_stride


class _BodySet:
    """an ow_bodies handle with the counts it was created with (WaveGenerator.bodies_create)"""

    def __init__(self, handle, num_bodies, num_points):
        self.handle, self.num_bodies, self.num_points = handle, num_bodies, num_points


class _Mesh:
    """an ow_mesh handle with the counts it was created with (WaveGenerator.mesh_create)"""

    def __init__(self, handle, num_vertices, num_triangles):
        self.handle, self.num_vertices, self.num_triangles = handle, num_vertices, num_triangles


class _Spray:
    """an ow_spray handle with the amount it was created with (WaveGenerator.spray_create)"""

    def __init__(self, handle, amount):
        self.handle, self.amount = handle, amount


class _SprayMaterial:
    """a billboard material on the device (WaveGenerator.spray_material_create)"""

    def __init__(self, handle):
        self.handle = handle


class _Solid:
    """a solid shape (WaveGenerator.solid_create)"""

    def __init__(self, handle, num_vertices, num_triangles):
        self.handle, self.num_vertices, self.num_triangles = handle, num_vertices, num_triangles


class Sky:
    """a device-resident panorama (ow_sky_create): WaveGenerator.sky_create() makes it, sky_destroy() ends it"""

    def __init__(self, handle, width, height):
        self.handle, self.width, self.height = handle, width, height


class Radiance:
    """a device-resident radiance pyramid of a sky (ow_radiance_create): WaveGenerator.radiance_create() makes it, radiance_destroy() ends it"""

    def __init__(self, handle, levels):
        self.handle, self.levels = handle, levels


class ShadowMap:
    """a device-resident sun shadow map (ow_shadow_map_create): WaveGenerator.shadow_map_create() makes it, shadow_map_destroy() ends it"""

    def __init__(self, handle, size):
        self.handle, self.size = handle, size


class WaveGenerator:
    """assets/water/wave_generator.gd.  Typical use, as in water.gd:89-91,112-114:

        gen = WaveGenerator(); gen.map_size = 1024; gen.init_gpu(max(2, len(parameters)))
        gen.update(delta, parameters)          # once per simulation tick
        gen._process(frame_delta)              # once per rendered frame (one cascade each)
    """

    def __init__(self):
        self.map_size = 0          # :8
        self.context = None        # :9  (ow_context*)
        self.descriptors = {}      # :11
        self.pass_parameters = []  # :14
        self._lib = None
        self.depth = DEPTH
        self.debug_f32 = False
        self.kernels = None           # None = runtime picks per batch; "standard" / "layer_parallel" pin the kernel family
        self.tick_groups = True        # False: run() keeps one pair of launches per tick (OW_FLAG_NO_TICK_GROUPS)
        self.run_as_calls = False      # True: run() issues its ticks as update_all() calls, one per tick (OW_FLAG_RUN_AS_CALLS)
        self.run_as_reference = False  # True: run() issues update() + one _process() per cascade, tick by tick (OW_FLAG_RUN_AS_REFERENCE_SCHEDULE)
        self.always_regenerate_spectrum = False  # True: every dirty flag launches the spectrum kernel, as the reference does (OW_FLAG_ALWAYS_REGENERATE_SPECTRUM)
        self.lazy_scratch = False      # True: ow_create allocates one batch of scratch, the look-ahead's share on first use (OW_FLAG_LAZY_SCRATCH)
        self.bodies_kernels = None     # None = the runtime picks per bodies_step() call; "fused" / "split" pin the shape (OW_FLAG_BODIES_FUSED / _SPLIT)
        self.single_stream = False     # True: tick-pair launches of four 1024^2 cascades stay whole, on the one stream (OW_FLAG_SINGLE_STREAM; default: two chains on two streams)
        self.group_forms = (None, None)  # tests: pin the tick groups' work-item forms -- ("lp" | "compact", "plain" | "pipe"); None = the runtime's choice
        self.device_id = -1
        self.stream = None
        self.external_maps = (None, None)  # optional caller-owned device buffers (displacement, normal)
        self.num_cascades = 0

    @property
    def pass_num_cascades_remaining(self):  # :15
        return self._lib.ow_cascades_remaining(self.context) if self.context else 0

    # ---- init_gpu (:17-54) ------------------------------------------------------------------------
    def init_gpu(self, num_cascades):
        self._lib = _lib.load()
        if self.context:
            self.free()
        cfg = ow_config(map_size=int(self.map_size), num_cascades=int(num_cascades), device_id=self.device_id,
                        depth=float(self.depth), stream=self.stream, displacement_map=self.external_maps[0],
                        normal_map=self.external_maps[1], flags=(OW_FLAG_DEBUG_F32 if self.debug_f32 else 0) | {None: 0, "lp": OW_FLAG_GROUP_P1_LP, "compact": OW_FLAG_GROUP_P1_COMPACT}[self.group_forms[0]] |
                        {None: 0, "plain": OW_FLAG_GROUP_P2_PLAIN, "pipe": OW_FLAG_GROUP_P2_PIPE}[self.group_forms[1]] | (0 if self.tick_groups else OW_FLAG_NO_TICK_GROUPS) | (OW_FLAG_RUN_AS_CALLS if self.run_as_calls else 0) | (OW_FLAG_RUN_AS_REFERENCE_SCHEDULE if self.run_as_reference else 0) |
                        (OW_FLAG_ALWAYS_REGENERATE_SPECTRUM if self.always_regenerate_spectrum else 0) | (OW_FLAG_LAZY_SCRATCH if self.lazy_scratch else 0) | (OW_FLAG_SINGLE_STREAM if self.single_stream else 0) |
                        {None: 0, "fused": _lib.OW_FLAG_BODIES_FUSED, "split": _lib.OW_FLAG_BODIES_SPLIT}[self.bodies_kernels] |
                        {None: 0, "standard": OW_FLAG_KERNELS_STANDARD, "layer_parallel": OW_FLAG_KERNELS_LAYER_PARALLEL,
                               "compact": OW_FLAG_KERNELS_COMPACT,
                               "layer_parallel_compact": OW_FLAG_KERNELS_LAYER_PARALLEL | OW_FLAG_KERNELS_COMPACT}[self.kernels])
        ctx = C.c_void_p()
        _lib.check(self._lib.ow_create(C.byref(cfg), C.byref(ctx)))
        self.context = ctx
        self.num_cascades = int(num_cascades)
        d, n, stride = C.c_void_p(), C.c_void_p(), C.c_size_t()
        _lib.check(self._lib.ow_get_device_ptrs(ctx, C.byref(d), C.byref(n), C.byref(stride)))
        self.descriptors = {"displacement_map": _Descriptor(d.value, stride.value),
                            "normal_map": _Descriptor(n.value, stride.value)}

    # ---- _process (:56-63) --------------------------------------------------------------------------
    def _process(self, delta=0.0):
        if not self.context or self.pass_num_cascades_remaining == 0:
            return
        idx = self.pass_num_cascades_remaining - 1
        self._push_live(idx)                                      # parameter objects are live in the reference
        _lib.check(self._lib.ow_process(self.context))
        self.pass_parameters[idx].should_generate_spectrum = False  # :72

    def _push_live(self, idx):
        """the context holds a COPY of the armed records (a C caller's memory is borrowed during a call only); the reference
        reads the live object when it processes a cascade, so the object's current fields are pushed right before"""
        c = ow_cascade_params()
        self.pass_parameters[idx]._pack(c)
        _lib.check(self._lib.ow_set_cascade_params(self.context, idx, C.byref(c)))

    # ---- update (:90-109) ------------------------------------------------------------------------------
    def _arm(self, fn, delta, parameters, drains_all):
        assert len(parameters) != 0                               # :91
        if not self.context:
            self.init_gpu(max(2, len(parameters)))                # :92-93
        leftovers = self.pass_parameters[:self.pass_num_cascades_remaining]
        for i in range(len(leftovers)):                           # the flush (:94-98) sees the live parameter objects
            self._push_live(i)
        new_c = (ow_cascade_params * len(parameters))()
        for p, c in zip(parameters, new_c):
            p._pack(c)
            if any(p is q for q in leftovers):                    # flushed by this very call: its spectrum is regenerated there (:72)
                c.should_generate_spectrum = 0
        _lib.check(fn(self.context, float(delta), new_c, len(parameters)))
        for q in leftovers:
            q.should_generate_spectrum = False
        for p, c in zip(parameters, new_c):                       # time and the foam rates advance inside the objects (:103-106)
            p.time, p.foam_grow_rate, p.foam_decay_rate = c.time, c.foam_grow_rate, c.foam_decay_rate
            if drains_all:
                p.should_generate_spectrum = False
        self.pass_parameters = list(parameters)

    def update(self, delta, parameters):
        self._arm(self._lib.ow_update if self._lib else _lib.load().ow_update, delta, parameters, False)

    def update_all(self, delta, parameters):
        """throughput mode (not in the reference): update() + every cascade in one pair of launches"""
        self._arm(self._lib.ow_update_all if self._lib else _lib.load().ow_update_all, delta, parameters, True)

    def run(self, delta, parameters, frames):
        """throughput mode: `frames` update_all() ticks enqueued back to back by the C runtime"""
        fn = self._lib.ow_run if self._lib else _lib.load().ow_run
        self._arm(lambda ctx, d, arr, cnt: fn(ctx, d, arr, cnt, int(frames)), delta, parameters, True)

    # ---- teardown (:111-113) -------------------------------------------------------------------------------
    def free(self):
        if self.context:
            self._lib.ow_destroy(self.context)
            self.context = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    # ---- statics (:116-121) -----------------------------------------------------------------------------------
    @staticmethod
    def JONSWAP_alpha(wind_speed=20.0, fetch_length=550e3):
        return _lib.load().ow_jonswap_alpha(wind_speed, fetch_length)

    @staticmethod
    def JONSWAP_peak_angular_frequency(wind_speed=20.0, fetch_length=550e3):
        return _lib.load().ow_jonswap_peak_angular_frequency(wind_speed, fetch_length)

    # ---- host read-back helpers (RenderingDevice.texture_get_data equivalents) ------------------------------
    def sync(self):
        _lib.check(self._lib.ow_sync(self.context))

    def debug_inject_fault(self, bits):
        """test hook (ow_debug_inject_fault): fault bits for the next batch only"""
        _lib.check(self._lib.ow_debug_inject_fault(self.context, int(bits)))

    def get_maps(self, cascade):
        n = self.map_size
        disp, norm = np.empty((n, n, 4), np.float16), np.empty((n, n, 4), np.float16)
        _lib.check(self._lib.ow_get_maps(self.context, cascade, disp.ctypes.data, norm.ctypes.data))
        return disp, norm

    def set_normal_map(self, cascade, normal):
        a = np.ascontiguousarray(normal, np.float16)
        assert a.shape == (self.map_size, self.map_size, 4)
        _lib.check(self._lib.ow_set_normal_map(self.context, cascade, a.ctypes.data))

    # ---- hand-off to a host-side consumer: the bytes for RenderingDevice.texture_update (water.gd:95-100) --------
    def readback_begin(self, cascades):
        """Start the asynchronous copy of the given layers (iterable of indices) into the context's page-locked
        staging memory; returns at once, later updates overlap the PCIe transfer."""
        mask = 0
        for i in cascades:
            mask |= 1 << int(i)
        _lib.check(self._lib.ow_readback_begin(self.context, mask))

    def readback_wait(self, cascade):
        """(displacement, normal) of one layer as float16 [N][N][4] VIEWS of the staging memory: valid until the next
        readback_begin of that layer (or free())."""
        d, m = C.c_void_p(), C.c_void_p()
        _lib.check(self._lib.ow_readback_wait(self.context, cascade, C.byref(d), C.byref(m)))
        n = self.map_size
        view = lambda p: np.frombuffer((C.c_uint16 * (n * n * 4)).from_address(p.value), np.float16).reshape(n, n, 4)
        return view(d), view(m)

    # ---- consumer-side sampling on the device (water.gdshader:27-39,72-82; sea_spray_particle.gdshader:78-96) ----
    SURFACE_SAMPLE = np.dtype([("displacement", np.float32, 3), ("gradient", np.float32, 2), ("gradient_scaled", np.float32, 2),
                               ("foam", np.float32), ("normal_factor", np.float32), ("foam_factor", np.float32),
                               ("scale_factor", np.float32), ("spray_active", np.int32), ("gradient_fragment", np.float32, 2),
                               ("foam_fragment", np.float32), ("reserved", np.float32)])

    def sample_surface(self, world_xz, map_scales):
        """Evaluate the water vertex/fragment sums and the sea-spray spawn mask at world points [P][2] (x, z);
        map_scales [C][4] as built by Water.map_scales() (water.gd:105-109).  Returns a structured array."""
        xz = np.ascontiguousarray(world_xz, np.float32).reshape(-1, 2)
        sc = _scales(map_scales)
        out = np.zeros(len(xz), self.SURFACE_SAMPLE)
        _lib.check(self._lib.ow_sample_surface(self.context, xz.ctypes.data, len(xz), sc.ctypes.data, len(sc), out.ctypes.data))
        return out

    # ---- the water above a world point: p + f(p) D(p) = q solved on the device (include/ocean_waves.h ow_query_surface) ----
    SURFACE_QUERY = np.dtype([("p", np.float32, 2), ("residual", np.float32), ("iterations", np.int32), ("evaluations", np.int32),
                              ("converged", np.int32), ("falloff", np.float32), ("height", np.float32), ("normal", np.float32, 3),
                              ("world_xz", np.float32, 2), ("reserved", np.int32, 3), ("sample", SURFACE_SAMPLE)])

    @staticmethod
    def query_options(options=None):
        """None, an _lib.ow_query_options, or a dict of max_iterations / tolerance / falloff_center ((x, z): the camera position
        of water.gdshader:29's distance falloff) -> ow_query_options, or None for the defaults"""
        if options is None or isinstance(options, _lib.ow_query_options):
            return options
        unknown = set(options) - {"max_iterations", "tolerance", "falloff_center"}
        if unknown:
            raise ValueError(f"unknown query options {sorted(unknown)}")
        o = _lib.ow_query_options(max_iterations=int(options.get("max_iterations", 0)), tolerance=float(options.get("tolerance", 0.0)))
        if options.get("falloff_center") is not None:
            o.flags = _lib.OW_QUERY_DISTANCE_FALLOFF
            o.falloff_center_xz[0], o.falloff_center_xz[1] = (float(v) for v in options["falloff_center"])
        return o

    def query_surface(self, world_xz, map_scales, options=None):
        """Where the rendered water is above world points [P][2] (x, z): the undisplaced point p, the residual, convergence, the
        rendered height and normal, and the full sample_surface record at p.  Returns a structured array (SURFACE_QUERY)."""
        xz = np.ascontiguousarray(world_xz, np.float32).reshape(-1, 2)
        sc = _scales(map_scales)
        out = np.zeros(len(xz), self.SURFACE_QUERY)
        o = self.query_options(options)
        _lib.check(self._lib.ow_query_surface(self.context, xz.ctypes.data, len(xz), sc.ctypes.data, len(sc),
                                              _ref(o), out.ctypes.data))
        return out

    def query_surface_async(self, xz_device, map_scales, out_device, options=None, count=None):
        """The query over DEVICE buffers, enqueued in the generator's stream order without synchronising: xz_device holds 2 * count
        float32 (x, z pairs), out_device room for count 128-byte records.  Each is anything with a data_ptr() (a torch tensor) or an
        integer address; count defaults to xz_device.numel() // 2."""
        if count is None:
            if not hasattr(xz_device, "numel"):
                raise ValueError("count is needed for a raw device address")
            count = int(xz_device.numel()) // 2
        _check_device_size(out_device, count, self.SURFACE_QUERY.itemsize)
        sc = _scales(map_scales)
        o = self.query_options(options)
        _lib.check(self._lib.ow_query_surface_async(self.context, _addr(xz_device), int(count), sc.ctypes.data, len(sc),
                                                    _ref(o), _addr(out_device)))

    # ---- buoyancy: per-body force and torque from hull points, on the device (include/ocean_waves.h ow_buoyancy) ----
    BUOYANCY_BODY = np.dtype([("transform", np.float32, 12), ("linear_velocity", np.float32, 3), ("angular_velocity", np.float32, 3),
                              ("point_offset", np.int32), ("point_count", np.int32), ("linear_drag", np.float32), ("quadratic_drag", np.float32),
                              ("reserved", np.uint32, 2)])
    HULL_POINT = np.dtype([("local", np.float32, 3), ("volume", np.float32), ("half_height", np.float32), ("body", np.int32),
                           ("reserved", np.uint32, 2)])
    BUOYANCY_OPTIONS = np.dtype([("query", [("max_iterations", np.int32), ("tolerance", np.float32), ("flags", np.uint32),
                                            ("falloff_center_xz", np.float32, 2), ("reserved", np.uint32, 3)]),
                                 ("density", np.float32), ("gravity", np.float32), ("water_level", np.float32), ("flags", np.uint32),
                                 ("reserved", np.uint32, 4)])
    BUOYANCY_POINT = np.dtype([("world", np.float32, 3), ("height", np.float32), ("depth", np.float32), ("submerged", np.float32),
                               ("force", np.float32, 3), ("p", np.float32, 2), ("residual", np.float32), ("iterations", np.int32),
                               ("evaluations", np.int32), ("converged", np.int32), ("body", np.int32)])
    BUOYANCY_RESULT = np.dtype([("force", np.float32, 3), ("torque", np.float32, 3), ("submerged_volume", np.float32),
                                ("center_of_buoyancy", np.float32, 3), ("wetted_points", np.int32), ("unconverged_points", np.int32),
                                ("invalid_points", np.int32), ("max_residual", np.float32), ("reserved", np.uint32, 2)])

    @classmethod
    def buoyancy_options(cls, options=None):
        """None, an _lib.ow_buoyancy_options, or a dict of density / gravity / water_level / warm_start (bool) / water_velocity (bool: drag
        relative to the moving surface) and the query_options keys -> ow_buoyancy_options, or None for the defaults"""
        if options is None or isinstance(options, _lib.ow_buoyancy_options):
            return options
        own = {"density", "gravity", "water_level", "warm_start", "water_velocity"}
        q = cls.query_options({k: v for k, v in options.items() if k not in own})
        flags = (_lib.OW_BUOYANCY_WARM_START if options.get("warm_start") else 0) | (_lib.OW_BUOYANCY_WATER_VELOCITY if options.get("water_velocity") else 0)
        o = _lib.ow_buoyancy_options(density=float(options.get("density", 0.0)), gravity=float(options.get("gravity", 0.0)),
                                     water_level=float(options.get("water_level", 0.0)), flags=flags)
        if q is not None:
            o.query = q
        return o

    @classmethod
    def box_hull(cls, size, divisions, body=0, center=(0.0, 0.0, 0.0)):
        """A box of size (x, y, z) metres centred at `center` (body space) voxelised into divisions (i, j, k) cells: one hull point per
        cell at its centre, volume = the cell's volume, half_height = half the cell's height.  Returns HULL_POINT records of `body`."""
        size = np.asarray(size, np.float64)
        div = np.asarray(divisions, np.int64)
        cell = size / div
        axes = [(np.arange(d) + 0.5) * c - s / 2 + o for d, c, s, o in zip(div, cell, size, center)]
        X, Y, Z = np.meshgrid(*axes, indexing="ij")
        out = np.zeros(X.size, cls.HULL_POINT)
        out["local"] = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
        out["volume"] = np.prod(cell)
        out["half_height"] = cell[1] / 2
        out["body"] = body
        return out

    def buoyancy(self, bodies, hull, map_scales, options=None, points=None):
        """Force, torque, submerged volume and centre of buoyancy per body (BUOYANCY_RESULT records) for BUOYANCY_BODY records over
        HULL_POINT records, on the device.  points: None, or a BUOYANCY_POINT array of len(hull) that receives the per-point records
        (and holds the previous step's for the warm start, options {"warm_start": True})."""
        b = np.ascontiguousarray(bodies, self.BUOYANCY_BODY)
        h = np.ascontiguousarray(hull, self.HULL_POINT)
        sc = _scales(map_scales)
        if points is not None and (not isinstance(points, np.ndarray) or points.dtype != self.BUOYANCY_POINT or len(points) != len(h)
                                   or not points.flags.c_contiguous):
            raise ValueError(f"points must be a contiguous BUOYANCY_POINT array of {len(h)} records")
        out = np.zeros(len(b), self.BUOYANCY_RESULT)
        o = self.buoyancy_options(options)
        _lib.check(self._lib.ow_buoyancy(self.context, b.ctypes.data, len(b), h.ctypes.data, len(h), sc.ctypes.data, len(sc),
                                         _ref(o), out.ctypes.data, points.ctypes.data if points is not None else None))
        return out

    def buoyancy_async(self, bodies_device, hull_device, map_scales, results_device, points_device, options=None, num_bodies=None,
                       num_points=None):
        """ow_buoyancy_async over DEVICE buffers (torch tensors or integer addresses), enqueued in the generator's stream order without
        synchronising.  The counts default to the tensors' byte sizes over the record sizes."""
        def records(x, dtype, given, name):
            if given is not None:
                return int(given)
            if not hasattr(x, "numel"):
                raise ValueError(f"{name} is needed for a raw device address")
            return int(x.numel() * x.element_size()) // dtype.itemsize
        nb = records(bodies_device, self.BUOYANCY_BODY, num_bodies, "num_bodies")
        npts = records(hull_device, self.HULL_POINT, num_points, "num_points")
        for x, n, dt, name in ((results_device, nb, self.BUOYANCY_RESULT, "results_device"), (points_device, npts, self.BUOYANCY_POINT, "points_device")):
            _check_device_size(x, n, dt.itemsize, name)
        sc = _scales(map_scales)
        o = self.buoyancy_options(options)
        _lib.check(self._lib.ow_buoyancy_async(self.context, _addr(bodies_device), nb, _addr(hull_device), npts, sc.ctypes.data, len(sc),
                                               _ref(o), _addr(results_device), _addr(points_device)))

    # ---- floating bodies stepped on the device (include/ocean_waves.h ow_bodies_step) ----
    RIGID_BODY = np.dtype([("position", np.float64, 3), ("orientation", np.float64, 4), ("linear_velocity", np.float64, 3),
                           ("angular_velocity", np.float64, 3), ("mass", np.float64), ("inverse_inertia", np.float64, 3),
                           ("applied_force", np.float64, 3), ("applied_torque", np.float64, 3), ("linear_drag", np.float32),
                           ("quadratic_drag", np.float32), ("point_offset", np.int32), ("point_count", np.int32), ("reserved", np.uint32, 2)])
    BODIES_OPTIONS = np.dtype([("buoyancy", BUOYANCY_OPTIONS), ("reserved", np.uint32, 4)])

    @staticmethod
    def box_mass_properties(size, density):
        """(mass, inverse principal inertia) of a solid box of size (x, y, z) metres and uniform density (kg/m^3) about its centre"""
        sx, sy, sz = (float(v) for v in size)
        mass = density * sx * sy * sz
        inertia = (mass / 12.0 * (sy * sy + sz * sz), mass / 12.0 * (sx * sx + sz * sz), mass / 12.0 * (sx * sx + sy * sy))
        return mass, tuple(1.0 / i for i in inertia)

    @classmethod
    def bodies_options(cls, options=None):
        """None, an _lib.ow_bodies_options, or what buoyancy_options() takes -> ow_bodies_options, or None for the defaults"""
        if options is None or isinstance(options, _lib.ow_bodies_options):
            return options
        o = _lib.ow_bodies_options()
        o.buoyancy = cls.buoyancy_options(options)
        return o

    def bodies_create(self, bodies, hull):
        """A device-resident body set from RIGID_BODY records and HULL_POINT records; returns a _BodySet (bodies_destroy() it before free())"""
        b = np.ascontiguousarray(bodies, self.RIGID_BODY)
        h = np.ascontiguousarray(hull, self.HULL_POINT)
        out = C.c_void_p()
        _lib.check(self._lib.ow_bodies_create(self.context, b.ctypes.data, len(b), h.ctypes.data, len(h), C.byref(out)))
        return _BodySet(out, len(b), len(h))

    def _destroy(self, obj, fn):
        """what every *_destroy does: the handle object is spent afterwards, a second destroy of it does nothing"""
        if obj.handle:
            fn(self.context, obj.handle)
            obj.handle = None

    def bodies_destroy(self, bodies_set):
        self._destroy(bodies_set, self._lib.ow_bodies_destroy)

    def bodies_step(self, bodies_set, map_scales, substeps, dt, options=None):
        """`substeps` substeps of dt seconds, enqueued in the generator's stream order without synchronising"""
        sc = _scales(map_scales)
        o = self.bodies_options(options)
        _lib.check(self._lib.ow_bodies_step(self.context, bodies_set.handle, sc.ctypes.data, len(sc), _ref(o), int(substeps),
                                            float(dt)))

    def bodies_state(self, bodies_set, first=0, count=None):
        """RIGID_BODY records of bodies [first, first + count) (count None: up to the last one); synchronises"""
        if count is None:
            count = bodies_set.num_bodies - first
        out = np.zeros(count, self.RIGID_BODY)
        _lib.check(self._lib.ow_bodies_get_state(self.context, bodies_set.handle, int(first), int(count), out.ctypes.data))
        return out

    def bodies_set_state(self, bodies_set, records, first=0):
        r = np.ascontiguousarray(records, self.RIGID_BODY)
        _lib.check(self._lib.ow_bodies_set_state(self.context, bodies_set.handle, int(first), len(r), r.ctypes.data))

    def bodies_results(self, bodies_set, first=0, count=None):
        """BUOYANCY_RESULT records of the last substep; synchronises"""
        if count is None:
            count = bodies_set.num_bodies - first
        out = np.zeros(count, self.BUOYANCY_RESULT)
        _lib.check(self._lib.ow_bodies_get_results(self.context, bodies_set.handle, int(first), int(count), out.ctypes.data))
        return out

    def bodies_device_ptrs(self, bodies_set):
        """device addresses of the pose records (BUOYANCY_BODY, Transform3D layout), the results and the per-point records"""
        b, r, p = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.check(self._lib.ow_bodies_get_device_ptrs(self.context, bodies_set.handle, C.byref(b), C.byref(r), C.byref(p)))
        return b.value, r.value, p.value

    def bodies_stats(self, bodies_set, faulted=True):
        """dict of substeps, fused_launches, split_calls and (synchronising) faulted_bodies"""
        v = [C.c_uint64() for _ in range(4)]
        _lib.check(self._lib.ow_bodies_stats(self.context, bodies_set.handle, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(v[3]) if faulted else None))
        out = {"substeps": v[0].value, "fused_launches": v[1].value, "split_calls": v[2].value}
        if faulted:
            out["faulted_bodies"] = v[3].value
        return out

    def sync_stats(self):
        """stream synchronisations the library has made on this thread since init_gpu (ow_sync_stats); does not synchronise"""
        v = C.c_uint64()
        _lib.check(self._lib.ow_sync_stats(self.context, C.byref(v)))
        return v.value

    # ---- ray casts against the rendered water, on the device (include/ocean_waves.h ow_raycast_surface) ----
    RAY = np.dtype([("origin", np.float32, 3), ("max_distance", np.float32), ("direction", np.float32, 3), ("reserved", np.uint32)])
    RAYCAST_OPTIONS = np.dtype([("query", BUOYANCY_OPTIONS.fields["query"][0]), ("water_level", np.float32), ("sample_spacing", np.float32),
                                ("tolerance", np.float32), ("max_samples", np.int32), ("reserved", np.uint32, 4)])
    RAYCAST_HIT = np.dtype([("t", np.float32), ("position", np.float32, 3), ("residual", np.float32), ("status", np.int32),
                            ("samples", np.int32), ("rounds", np.int32), ("slab_half_height", np.float32), ("t_enter", np.float32),
                            ("t_exit", np.float32), ("reserved", np.uint32, 5), ("query", SURFACE_QUERY)])

    @classmethod
    def rays(cls, origins, directions, max_distance):
        """RAY records from origins [R][3], directions [R][3] (any non-zero length) and max_distance (a scalar or [R]).  Godot's
        intersect_ray(from, to): origin = from, direction = to - from, max_distance = |to - from|."""
        o = np.asarray(origins, np.float32).reshape(-1, 3)
        out = np.zeros(len(o), cls.RAY)
        out["origin"] = o
        out["direction"] = np.asarray(directions, np.float32).reshape(-1, 3)
        out["max_distance"] = max_distance
        return out

    @classmethod
    def raycast_options(cls, options=None):
        """None, an _lib.ow_raycast_options, or a dict of water_level / sample_spacing / tolerance / max_samples and the query_options
        keys (query_tolerance for the query's own tolerance) -> ow_raycast_options, or None for the defaults"""
        if options is None or isinstance(options, _lib.ow_raycast_options):
            return options
        own = {"water_level", "sample_spacing", "tolerance", "max_samples", "query_tolerance"}
        q = {k: v for k, v in options.items() if k not in own}
        if "query_tolerance" in options:
            q["tolerance"] = options["query_tolerance"]
        qo = cls.query_options(q) if q else None
        o = _lib.ow_raycast_options(water_level=float(options.get("water_level", 0.0)), sample_spacing=float(options.get("sample_spacing", 0.0)),
                                    tolerance=float(options.get("tolerance", 0.0)), max_samples=int(options.get("max_samples", 0)))
        if qo is not None:
            o.query = qo
        return o

    def raycast_surface(self, rays, map_scales, options=None):
        """Where each RAY record first meets the rendered water: t, the position, the status bits (_lib.OW_RAY_*), the slab searched
        and the SURFACE_QUERY record at the hit.  Returns a structured array (RAYCAST_HIT)."""
        r = np.ascontiguousarray(rays, self.RAY)
        sc = _scales(map_scales)
        out = np.zeros(len(r), self.RAYCAST_HIT)
        o = self.raycast_options(options)
        _lib.check(self._lib.ow_raycast_surface(self.context, r.ctypes.data, len(r), sc.ctypes.data, len(sc),
                                                _ref(o), out.ctypes.data))
        return out

    def raycast_surface_async(self, rays_device, map_scales, out_device, options=None, count=None):
        """The ray casts over DEVICE buffers, enqueued in the generator's stream order without synchronising: rays_device holds count
        32-byte RAY records, out_device room for count 192-byte records.  Each is anything with a data_ptr() (a torch tensor) or an
        integer address; count defaults to the byte size of rays_device over 32."""
        if count is None:
            if not hasattr(rays_device, "numel"):
                raise ValueError("count is needed for a raw device address")
            count = int(rays_device.numel() * rays_device.element_size()) // self.RAY.itemsize
        _check_device_size(out_device, count, self.RAYCAST_HIT.itemsize)
        sc = _scales(map_scales)
        o = self.raycast_options(options)
        _lib.check(self._lib.ow_raycast_surface_async(self.context, _addr(rays_device), int(count), sc.ctypes.data, len(sc),
                                                      _ref(o), _addr(out_device)))

    # ---- the water's velocity: V = dD/dt per layer, and the surface's velocity above world points (include/ocean_waves.h ow_update_velocity) ----
    SURFACE_VELOCITY = np.dtype([("velocity", np.float32, 3), ("height", np.float32), ("p", np.float32, 2), ("converged", np.int32),
                                 ("reserved", np.uint32)])

    def update_velocity(self, cascades=None):
        """enqueue the refresh of the stale velocity layers among `cascades` (indices; None = all), without synchronising"""
        mask = (1 << self.num_cascades) - 1 if cascades is None else sum(1 << int(i) for i in cascades)
        _lib.check(self._lib.ow_update_velocity(self.context, mask))

    def velocity_ptrs(self):
        """(device address of the velocity array, layer stride in bytes), every computed layer refreshed first"""
        p, st = C.c_void_p(), C.c_size_t()
        _lib.check(self._lib.ow_get_velocity_ptrs(self.context, C.byref(p), C.byref(st)))
        return p.value, st.value

    def velocity_map(self, cascade):
        """layer `cascade` of the velocity array as FP16 [N][N][4]: (dD_x/dt, dD_y/dt, dD_z/dt, 0) in m/s, before displacement_scale"""
        n = self.map_size
        out = np.empty((n, n, 4), np.float16)
        _lib.check(self._lib.ow_get_velocity_map(self.context, int(cascade), out.ctypes.data))
        return out

    def velocity_stats(self):
        """(computed, skipped): velocity layers computed, and layers asked for that were current already"""
        a, b = C.c_uint64(), C.c_uint64()
        _lib.check(self._lib.ow_velocity_stats(self.context, C.byref(a), C.byref(b)))
        return a.value, b.value

    def query_velocity(self, world_xz, map_scales, options=None):
        """The velocity of the rendered surface above world points [P][2] (x, z), with ow_query_surface's height, p and convergence.
        Returns a structured array (SURFACE_VELOCITY)."""
        xz = np.ascontiguousarray(world_xz, np.float32).reshape(-1, 2)
        sc = _scales(map_scales)
        out = np.zeros(len(xz), self.SURFACE_VELOCITY)
        o = self.query_options(options)
        _lib.check(self._lib.ow_query_velocity(self.context, xz.ctypes.data, len(xz), sc.ctypes.data, len(sc),
                                               _ref(o), out.ctypes.data))
        return out

    def query_velocity_async(self, xz_device, map_scales, out_device, options=None, count=None):
        """query_velocity over DEVICE buffers, as query_surface_async (out_device: room for count 32-byte records)"""
        if count is None:
            if not hasattr(xz_device, "numel"):
                raise ValueError("count is needed for a raw device address")
            count = int(xz_device.numel()) // 2
        _check_device_size(out_device, count, self.SURFACE_VELOCITY.itemsize)
        sc = _scales(map_scales)
        o = self.query_options(options)
        _lib.check(self._lib.ow_query_velocity_async(self.context, _addr(xz_device), int(count), sc.ctypes.data, len(sc),
                                                     _ref(o), _addr(out_device)))

    # ---- camera views of the water, on the device (include/ocean_waves.h ow_render_view) ----
    RENDER_PIXEL = np.dtype([("t", np.float32), ("status", np.int32), ("position", np.float32, 3), ("p", np.float32, 2), ("wave_height", np.float32),
                             ("gradient_fragment", np.float32, 2), ("foam_fragment", np.float32), ("dist", np.float32), ("foam_factor", np.float32),
                             ("albedo", np.float32, 3), ("normal", np.float32, 3), ("fresnel", np.float32), ("roughness", np.float32),
                             ("diffuse", np.float32, 3), ("specular", np.float32), ("color", np.float32, 3), ("reserved", np.uint32, 4)])
    _RENDER_OWN = ("water_color", "foam_color", "roughness", "normal_strength", "light_direction", "light_color", "ambient_color", "sky_color")

    @staticmethod
    def camera(position, basis, fov_y_degrees, width, height, max_distance):
        """an _lib.ow_camera from a position, Godot Transform3D basis rows (9 values or 3 x 3; the camera looks down its -Z, +Y is up),
        the vertical field of view in degrees, the image size and the length of each pixel's ray"""
        cam = _lib.ow_camera(max_distance=float(max_distance), fov_y_degrees=float(fov_y_degrees), width=int(width), height=int(height))
        cam.position[:] = [float(v) for v in position]
        cam.basis[:] = [float(v) for v in np.asarray(basis, np.float64).reshape(9)]
        return cam

    @classmethod
    def _set_material(cls, o, options):
        """the material and light keys render_options and mesh_options share (_RENDER_OWN), from the dict into the struct"""
        for k in cls._RENDER_OWN:
            if k in options:
                if k in ("roughness", "normal_strength"):
                    setattr(o, k, float(options[k]))
                else:
                    getattr(o, k)[:] = [float(v) for v in options[k]]

    @classmethod
    def _picture(cls, camera, pixels, want_rgba):
        """The host arrays of a synchronous picture call: ((H, W, 4) uint8 RGBA or None, (H, W) RENDER_PIXEL records or None).  pixels: None
        (no records), True (zeroed ones) or records to start from (copied; ValueError unless they have the image's shape).  The RGBA image is
        left out only where there are records and want_rgba is false."""
        h, w = max(int(camera.height), 0), max(int(camera.width), 0)
        big = h > _lib.OW_RENDER_MAX_SIDE or w > _lib.OW_RENDER_MAX_SIDE   # refused by the library: do not allocate for it
        shape = (1, 1) if big else (h, w)
        rec = None
        if pixels is True:
            rec = np.zeros(shape, cls.RENDER_PIXEL)
        elif pixels is not None:
            rec = np.array(pixels, cls.RENDER_PIXEL, copy=True, order="C")
            if not big and rec.shape != (h, w):
                raise ValueError(f"pixels is {rec.shape}, the camera's image {(h, w)}")
        rgba = np.zeros(shape + (4,), np.uint8) if want_rgba or rec is None else None
        return rgba, rec

    def _check_picture_buffers(self, camera, rgba_device, pixels_device):
        """the size checks of the asynchronous picture calls' device buffers"""
        count = int(camera.width) * int(camera.height)
        for buf, size in ((rgba_device, 4), (pixels_device, self.RENDER_PIXEL.itemsize)):
            _check_device_size(buf, count, size, "a device buffer", "pixels")

    @classmethod
    def render_options(cls, options=None, camera=None):
        """None, an _lib.ow_render_options, or a dict -> ow_render_options, or None for the defaults.  The dict starts from
        ow_render_options_default's values and may set water_color / foam_color / roughness / normal_strength / light_direction /
        light_color / ambient_color / sky_color and the raycast_options keys.  "falloff": True turns the shader's distance falloff on
        around the camera's x and z (falloff_center names another centre)."""
        if options is None or isinstance(options, _lib.ow_render_options):
            return options
        o = _lib.ow_render_options()
        _lib.load().ow_render_options_default(C.byref(o))
        ray = {k: v for k, v in options.items() if k not in cls._RENDER_OWN and k != "falloff"}
        if options.get("falloff") and ray.get("falloff_center") is None:
            if camera is None:
                raise ValueError("falloff without a falloff_center needs the camera")
            ray["falloff_center"] = (camera.position[0], camera.position[2])
        if ray:
            o.raycast = cls.raycast_options(ray)
        cls._set_material(o, options)
        return o

    def render_view(self, camera, map_scales, options=None, pixels=True):
        """The view of an ow_camera (WaveGenerator.camera): ((H, W, 4) uint8 RGBA, (H, W) structured RENDER_PIXEL records, or None with
        pixels=False), rows from the top."""
        sc = _scales(map_scales)
        o = self.render_options(options, camera)
        rgba, rec = self._picture(camera, True if pixels else None, True)
        _lib.check(self._lib.ow_render_view(self.context, C.byref(camera), sc.ctypes.data, len(sc), _ref(o),
                                            rgba.ctypes.data, rec.ctypes.data if pixels else None))
        return rgba, rec

    def render_view_async(self, camera, map_scales, rgba_device, pixels_device=None, options=None):
        """The view over DEVICE buffers, enqueued in the generator's stream order without synchronising: rgba_device holds H * W * 4 bytes,
        pixels_device H * W 128-byte records; each is anything with a data_ptr() (a torch tensor), an integer address, or None (not both)."""
        self._check_picture_buffers(camera, rgba_device, pixels_device)
        sc = _scales(map_scales)
        o = self.render_options(options, camera)
        _lib.check(self._lib.ow_render_view_async(self.context, C.byref(camera), sc.ctypes.data, len(sc), _ref(o),
                                                  _addr(rgba_device, True), _addr(pixels_device, True)))

    # ---- a displaced water mesh drawn for a camera, on the device (include/ocean_waves.h ow_mesh_*) ----
    MESH_VERTEX = np.dtype([("position", np.float32, 3), ("wave_height", np.float32), ("uv", np.float32, 2), ("distance_factor", np.float32),
                            ("reserved", np.uint32), ("view_position", np.float32, 3), ("flags", np.uint32)])
    _MESH_OWN = _RENDER_OWN + ("near", "cull_back", "lane_box", "falloff", "falloff_center")

    @staticmethod
    def clipmap_origin(camera_position, tile_size):
        """main.gd:34-37: where the water mesh is put for a camera -- ceil(camera.xz / tile) * tile, y = 0 -- as float32 (x, 0, z)"""
        xz = np.array([camera_position[0], camera_position[2]], np.float32)   # Vector3 is FP32
        t = np.float32(tile_size)
        out = np.ceil(xz / t) * t
        return np.array([out[0], 0.0, out[1]], np.float32)

    @classmethod
    def mesh_options(cls, options=None, camera=None):
        """None, an _lib.ow_mesh_options, or a dict -> ow_mesh_options, or None for the defaults.  The dict starts from
        ow_mesh_options_default's values and may set the shading keys of render_options, near, cull_back, lane_box and falloff_center;
        "falloff": True turns the shader's distance falloff on around the camera's x and z."""
        if options is None or isinstance(options, _lib.ow_mesh_options):
            return options
        unknown = [k for k in options if k not in cls._MESH_OWN]
        if unknown:
            raise ValueError(f"unknown mesh options {unknown}")
        o = _lib.ow_mesh_options()
        _lib.load().ow_mesh_options_default(C.byref(o))
        center = options.get("falloff_center")
        if options.get("falloff") and center is None:
            if camera is None:
                raise ValueError("falloff without a falloff_center needs the camera")
            center = (camera.position[0], camera.position[2])
        if center is not None:
            o.query_flags = _lib.OW_QUERY_DISTANCE_FALLOFF
            o.falloff_center_xz[:] = [float(v) for v in center]
        cls._set_material(o, options)
        if "near" in options:
            o.near = float(options["near"])
        if options.get("cull_back"):
            o.flags |= _lib.OW_MESH_CULL_BACK
        if "lane_box" in options:
            o.lane_box = int(options["lane_box"])
        return o

    def mesh_create(self, vertices, triangles):
        """A device-resident mesh from [V][3] local positions and [T][3] vertex indices; returns a _Mesh (mesh_destroy() it before free())"""
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
        out = C.c_void_p()
        _lib.check(self._lib.ow_mesh_create(self.context, v.ctypes.data, len(v), t.ctypes.data, len(t), C.byref(out)))
        return _Mesh(out, len(v), len(t))

    def mesh_destroy(self, mesh):
        self._destroy(mesh, self._lib.ow_mesh_destroy)

    def mesh_displace(self, mesh, origin, map_scales, options=None, camera=None):
        """The vertex stage alone: MESH_VERTEX records of every vertex (view_position only with a camera); synchronises"""
        sc = _scales(map_scales)
        org = np.ascontiguousarray(origin, np.float32).reshape(3)
        o = self.mesh_options(options, camera)
        out = np.zeros(mesh.num_vertices, self.MESH_VERTEX)
        _lib.check(self._lib.ow_mesh_displace(self.context, mesh.handle, org.ctypes.data, sc.ctypes.data, len(sc), _ref(o),
                                              _ref(camera), out.ctypes.data))
        return out

    def mesh_device_ptrs(self, mesh):
        """device addresses of the mesh's resident MESH_VERTEX records and of the context's visibility words (None before the first draw)"""
        v, w = C.c_void_p(), C.c_void_p()
        _lib.check(self._lib.ow_mesh_get_device_ptrs(self.context, mesh.handle, C.byref(v), C.byref(w)))
        return v.value, w.value

    def mesh_draw(self, mesh, camera, origin, map_scales, options=None, pixels=True):
        """The mesh as an ow_camera sees it: ((H, W, 4) uint8 RGBA, (H, W) RENDER_PIXEL records or None with pixels=False), rows from the
        top; a record's reserved[0] is the drawn triangle's index + 1."""
        sc = _scales(map_scales)
        org = np.ascontiguousarray(origin, np.float32).reshape(3)
        o = self.mesh_options(options, camera)
        rgba, rec = self._picture(camera, True if pixels else None, True)
        _lib.check(self._lib.ow_mesh_draw(self.context, mesh.handle, C.byref(camera), org.ctypes.data, sc.ctypes.data, len(sc),
                                          _ref(o), rgba.ctypes.data, rec.ctypes.data if pixels else None))
        return rgba, rec

    def mesh_draw_async(self, mesh, camera, origin, map_scales, rgba_device, pixels_device=None, options=None):
        """The draw over DEVICE buffers, enqueued in the generator's stream order without synchronising (render_view_async's buffers)"""
        self._check_picture_buffers(camera, rgba_device, pixels_device)
        sc = _scales(map_scales)
        org = np.ascontiguousarray(origin, np.float32).reshape(3)
        o = self.mesh_options(options, camera)
        _lib.check(self._lib.ow_mesh_draw_async(self.context, mesh.handle, C.byref(camera), org.ctypes.data, sc.ctypes.data, len(sc),
                                                _ref(o), _addr(rgba_device, True), _addr(pixels_device, True)))

    def mesh_stats(self, mesh):
        """dict of draws and, of the last draw (synchronising), the triangles skipped, culled, per_lane and cooperative"""
        v = [C.c_uint64() for _ in range(5)]
        _lib.check(self._lib.ow_mesh_stats(self.context, mesh.handle, *[C.byref(x) for x in v]))
        return dict(zip(("draws", "skipped", "culled", "per_lane", "cooperative"), (x.value for x in v)))

    # ---- the sea-spray particle emitter on the device (include/ocean_waves.h ow_spray_*) ----
    SPRAY_INSTANCE = np.dtype([("transform", np.float32, 12), ("custom", np.float32, 4)])
    SPRAY_PARTICLE = np.dtype([("start_pos", np.float32, 3), ("start_time", np.float32), ("particle_scale", np.float32, 3),
                               ("particle_lifetime", np.float32), ("custom_z", np.float32), ("scale_factor", np.float32), ("flags", np.uint32),
                               ("number", np.uint32)])
    _SPRAY_OWN = ("amount", "num_particles", "emitter_lifetime", "lifetime", "lifetime_randomness", "particle_scale", "random_seed",
                  "emission_transform", "start_time")

    @classmethod
    def spray_options(cls, options=None):
        """None, an _lib.ow_spray_options, or a dict -> ow_spray_options.  The dict starts from ow_spray_options_default's values (the
        reference scene's emitter) and may set amount, num_particles, emitter_lifetime, lifetime, lifetime_randomness, particle_scale,
        random_seed, emission_transform (3 x 4) and start_time."""
        if isinstance(options, _lib.ow_spray_options):
            return options
        options = options or {}
        unknown = [k for k in options if k not in cls._SPRAY_OWN]
        if unknown:
            raise ValueError(f"unknown spray options {unknown}")
        o = _lib.ow_spray_options()
        _lib.load().ow_spray_options_default(C.byref(o))
        for k, v in options.items():
            if k == "particle_scale":
                o.particle_scale[:] = [float(x) for x in np.asarray(v, np.float32).reshape(3)]
            elif k == "emission_transform":
                o.emission_transform[:] = [float(x) for x in np.asarray(v, np.float32).reshape(12)]
            elif k in ("amount", "num_particles", "random_seed"):
                setattr(o, k, int(v))
            else:
                setattr(o, k, float(v))
        return o

    def spray_create(self, options=None):
        """A device-resident emitter, every particle dormant; returns a _Spray (spray_destroy() it before free())"""
        o = self.spray_options(options)
        out = C.c_void_p()
        _lib.check(self._lib.ow_spray_create(self.context, C.byref(o), C.byref(out)))
        return _Spray(out, int(o.amount))

    def spray_destroy(self, spray):
        self._destroy(spray, self._lib.ow_spray_destroy)

    def spray_step(self, spray, delta, map_scales):
        """One frame of the emitter on the maps as they stand in the generator's stream order; enqueues and returns"""
        sc = _scales(map_scales)
        _lib.check(self._lib.ow_spray_step(self.context, spray.handle, float(delta), sc.ctypes.data, len(sc)))

    def spray_read(self, spray):
        """(SPRAY_INSTANCE[amount], SPRAY_PARTICLE[amount], draw list uint32[live_count]) as the last step left them; synchronises"""
        inst, part = np.zeros(spray.amount, self.SPRAY_INSTANCE), np.zeros(spray.amount, self.SPRAY_PARTICLE)
        draw, live = np.zeros(spray.amount, np.uint32), C.c_uint32()
        _lib.check(self._lib.ow_spray_read(self.context, spray.handle, inst.ctypes.data, part.ctypes.data, draw.ctypes.data, C.byref(live)))
        return inst, part, draw[:live.value].copy()

    def spray_live_count(self, spray):
        live = C.c_uint32()
        _lib.check(self._lib.ow_spray_read(self.context, spray.handle, None, None, None, C.byref(live)))
        return live.value

    def spray_device_ptrs(self, spray):
        """device addresses of the instances, the state records, the draw list and the live count"""
        v = [C.c_void_p() for _ in range(4)]
        _lib.check(self._lib.ow_spray_get_device_ptrs(self.context, spray.handle, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def spray_stats(self, spray):
        """dict of time, steps, restarts (the host's bookkeeping) and spawned, rejected (summed on the device; synchronises)"""
        v = [C.c_double()] + [C.c_uint64() for _ in range(4)]
        _lib.check(self._lib.ow_spray_stats(self.context, spray.handle, *[C.byref(x) for x in v]))
        return dict(zip(("time", "steps", "restarts", "spawned", "rejected"), (x.value for x in v)))

    # ---- the spray billboards drawn into a camera view (include/ocean_waves.h ow_billboard_*) ----
    _SPRAY_MATERIAL_OWN = ("foam_color", "max_alpha", "albedo_srgb", "dissolve_srgb")
    _SPRAY_DRAW_OWN = ("near", "background_color", "bin_side")

    @classmethod
    def spray_material_options(cls, options=None):
        """None, an _lib.ow_billboard_material_options, or a dict over ow_billboard_material_options_default's values (the reference scene's
        foam colour, max_alpha 0.666, both textures sRGB) that may set foam_color, max_alpha, albedo_srgb and dissolve_srgb"""
        if isinstance(options, _lib.ow_billboard_material_options):
            return options
        options = options or {}
        unknown = [k for k in options if k not in cls._SPRAY_MATERIAL_OWN]
        if unknown:
            raise ValueError(f"unknown spray material options {unknown}")
        o = _lib.ow_billboard_material_options()
        _lib.load().ow_billboard_material_options_default(C.byref(o))
        if "foam_color" in options:
            o.foam_color[:] = [float(v) for v in options["foam_color"]]
        if "max_alpha" in options:
            o.max_alpha = float(options["max_alpha"])
        for k in ("albedo_srgb", "dissolve_srgb"):
            if k in options:
                setattr(o, k, int(options[k]))
        return o

    @classmethod
    def spray_draw_options(cls, options=None):
        """None, an _lib.ow_billboard_draw_options, or a dict of near, background_color and bin_side -> ow_billboard_draw_options or None"""
        if options is None or isinstance(options, _lib.ow_billboard_draw_options):
            return options
        unknown = [k for k in options if k not in cls._SPRAY_DRAW_OWN]
        if unknown:
            raise ValueError(f"unknown spray draw options {unknown}")
        o = _lib.ow_billboard_draw_options()
        if "near" in options:
            o.near = float(options["near"])
        if "background_color" in options:
            o.background_color[:] = [float(v) for v in options["background_color"]]
        if "bin_side" in options:
            o.bin_side = int(options["bin_side"])
        return o

    def spray_material_create(self, albedo_rgba8, dissolve_rgba8, options=None):
        """A billboard material from two (H, W, 4) uint8 textures, uploaded once; returns a _SprayMaterial (spray_material_destroy() it
        before free())"""
        a, d = (np.ascontiguousarray(t, np.uint8) for t in (albedo_rgba8, dissolve_rgba8))
        for t in (a, d):
            if t.ndim != 3 or t.shape[2] != 4:
                raise ValueError("a texture is (height, width, 4) uint8")
        o = self.spray_material_options(options)
        out = C.c_void_p()
        _lib.check(self._lib.ow_billboard_material_create(self.context, C.byref(o), a.ctypes.data, a.shape[1], a.shape[0], d.ctypes.data, d.shape[1],
                                                          d.shape[0], C.byref(out)))
        return _SprayMaterial(out)

    def spray_material_destroy(self, material):
        self._destroy(material, self._lib.ow_billboard_material_destroy)

    def spray_draw(self, spray, material, camera, options=None, pixels=None, rgba=True):
        """The emitter's live particles blended over `pixels` ((H, W) RENDER_PIXEL records of mesh_draw or render_view; None: the options'
        background colour, no depth): ((H, W, 4) uint8 RGBA, the records rewritten or None); a record's reserved[1] counts the fragments
        blended, reserved[2] is the last one's particle index + 1.  Synchronises."""
        o = self.spray_draw_options(options)
        img, rec = self._picture(camera, pixels, rgba)
        _lib.check(self._lib.ow_billboard_draw(self.context, spray.handle, material.handle, C.byref(camera), _ref(o),
                                               rec.ctypes.data if rec is not None else None, img.ctypes.data if img is not None else None))
        return img, rec

    def spray_draw_instances(self, material, instances, time, camera, options=None, pixels=None, rgba=True):
        """spray_draw over a host array of SPRAY_INSTANCE records, drawn in array order, with TIME = time"""
        inst = np.ascontiguousarray(instances, self.SPRAY_INSTANCE).reshape(-1)
        o = self.spray_draw_options(options)
        img, rec = self._picture(camera, pixels, rgba)
        _lib.check(self._lib.ow_billboard_draw_instances(self.context, material.handle, inst.ctypes.data if len(inst) else None, len(inst), float(time),
                                                         C.byref(camera), _ref(o),
                                                         rec.ctypes.data if rec is not None else None, img.ctypes.data if img is not None else None))
        return img, rec

    def spray_draw_async(self, spray, material, camera, rgba_device, pixels_device=None, options=None):
        """The draw over DEVICE buffers (mesh_draw_async's), enqueued in the generator's stream order without synchronising; the records are
        read and rewritten in place"""
        self._check_picture_buffers(camera, rgba_device, pixels_device)
        o = self.spray_draw_options(options)
        _lib.check(self._lib.ow_billboard_draw_async(self.context, spray.handle, material.handle, C.byref(camera), _ref(o),
                                                     _addr(pixels_device, True), _addr(rgba_device, True)))

    def spray_draw_stats(self, counters=True):
        """dict of draws, the scratch bytes held and, with counters (synchronising), the billboards the last draw culled and drawn"""
        v = [C.c_uint64() for _ in range(4)]
        _lib.check(self._lib.ow_billboard_draw_stats(self.context, C.byref(v[0]), C.byref(v[1]) if counters else None, C.byref(v[2]) if counters else None,
                                                     C.byref(v[3])))
        keys = ("draws", "culled", "drawn", "scratch_bytes")
        return {k: x.value for k, x in zip(keys, v) if counters or k in ("draws", "scratch_bytes")}

    # ---- solids drawn into a camera view, on the device (include/ocean_waves.h ow_solid_*) ----
    _SOLID_OWN = ("near", "color", "light_direction", "light_color", "ambient_color", "background_color", "two_sided", "lane_box")

    @classmethod
    def solid_options(cls, options=None):
        """None, an _lib.ow_solid_options, or a dict over ow_solid_options_default's values (the reference scene's sun and ambient, a brown
        albedo) that may set near, color, light_direction, light_color, ambient_color, background_color, two_sided and lane_box"""
        if options is None or isinstance(options, _lib.ow_solid_options):
            return options
        unknown = [k for k in options if k not in cls._SOLID_OWN]
        if unknown:
            raise ValueError(f"unknown solid options {unknown}")
        o = _lib.ow_solid_options()
        _lib.load().ow_solid_options_default(C.byref(o))
        for k in ("color", "light_direction", "light_color", "ambient_color", "background_color"):
            if k in options:
                getattr(o, k)[:] = [float(v) for v in options[k]]
        if "near" in options:
            o.near = float(options["near"])
        if options.get("two_sided"):
            o.flags |= _lib.OW_SOLID_TWO_SIDED
        if "lane_box" in options:
            o.lane_box = int(options["lane_box"])
        return o

    def solid_create(self, vertices, triangles):
        """A device-resident shape from [V][3] local positions and [T][3] vertex indices (counter-clockwise seen from outside); returns a
        _Solid (solid_destroy() it before free())"""
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
        out = C.c_void_p()
        _lib.check(self._lib.ow_solid_create(self.context, v.ctypes.data, len(v), t.ctypes.data, len(t), C.byref(out)))
        return _Solid(out, len(v), len(t))

    def solid_destroy(self, solid):
        self._destroy(solid, self._lib.ow_solid_destroy)

    def solid_draw(self, solid, bodies_set, camera, options=None, pixels=None, rgba=True, first=0, count=None):
        """The shape at the resident poses of bodies [first, first + count) of a body set, drawn over `pixels` ((H, W) RENDER_PIXEL records of
        mesh_draw or render_view; None: the options' background colour, no depth): ((H, W, 4) uint8 RGBA, the records rewritten or None).  A
        record a solid wins carries OW_RAY_SOLID, reserved[0] the triangle's index + 1 and reserved[3] the instance's index + 1.
        Synchronises."""
        count = bodies_set.num_bodies - first if count is None else count
        o = self.solid_options(options)
        img, rec = self._picture(camera, pixels, rgba)
        _lib.check(self._lib.ow_solid_draw(self.context, solid.handle, bodies_set.handle, int(first), int(count), C.byref(camera), _ref(o),
                                           rec.ctypes.data if rec is not None else None, img.ctypes.data if img is not None else None))
        return img, rec

    def solid_draw_instances(self, solid, transforms, camera, options=None, pixels=None, rgba=True):
        """solid_draw over a host array of [count][12] transforms (basis rows, then the origin)"""
        t = np.ascontiguousarray(transforms, np.float32).reshape(-1, 12)
        o = self.solid_options(options)
        img, rec = self._picture(camera, pixels, rgba)
        _lib.check(self._lib.ow_solid_draw_instances(self.context, solid.handle, t.ctypes.data if len(t) else None, len(t), C.byref(camera), _ref(o),
                                                     rec.ctypes.data if rec is not None else None, img.ctypes.data if img is not None else None))
        return img, rec

    def solid_draw_async(self, solid, bodies_set, camera, rgba_device, pixels_device=None, options=None, first=0, count=None):
        """The draw over DEVICE buffers (mesh_draw_async's), enqueued in the generator's stream order without synchronising; the records are
        read and rewritten in place"""
        self._check_picture_buffers(camera, rgba_device, pixels_device)
        count = bodies_set.num_bodies - first if count is None else count
        o = self.solid_options(options)
        _lib.check(self._lib.ow_solid_draw_async(self.context, solid.handle, bodies_set.handle, int(first), int(count), C.byref(camera), _ref(o),
                                                 _addr(pixels_device, True), _addr(rgba_device, True)))

    def solid_draw_stats(self, counters=True):
        """dict of draws, the scratch bytes held and, with counters (synchronising), the instances the last draw skipped and the triangles
        it culled and drew"""
        v = [C.c_uint64() for _ in range(5)]
        _lib.check(self._lib.ow_solid_draw_stats(self.context, C.byref(v[0]), *(C.byref(x) if counters else None for x in v[1:4]), C.byref(v[4])))
        keys = ("draws", "skipped_instances", "culled", "drawn", "scratch_bytes")
        return {k: x.value for k, x in zip(keys, v) if counters or k in ("draws", "scratch_bytes")}

    # ---- the finishing stage: sky, fog, tonemap, sRGB (include/ocean_waves.h ow_sky_*, ow_environment_apply, ow_present) ----
    _SKY_OWN = ("srgb", "energy")
    _ENVIRONMENT_OWN = ("fog_mode", "density", "depth_begin", "depth_end", "depth_curve", "aerial_perspective", "sun_scatter", "light_color", "sun_color",
                        "sun_direction", "sky_color")
    _PRESENT_OWN = ("downsample", "tonemap", "exposure", "white", "srgb", "brightness", "contrast", "saturation")
    FOG_MODES = {"exponential": _lib.OW_FOG_EXPONENTIAL, "depth": _lib.OW_FOG_DEPTH}
    TONEMAPS = {"linear": _lib.OW_TONEMAP_LINEAR, "reinhard": _lib.OW_TONEMAP_REINHARD, "filmic": _lib.OW_TONEMAP_FILMIC}

    @staticmethod
    def _options(struct, default, own, options, what, names=None):
        """None or a struct pass; a dict is laid over the default's values (names: key -> {word: value} for the enumerations)"""
        if options is None or isinstance(options, struct):
            return options
        unknown = [k for k in options if k not in own]
        if unknown:
            raise ValueError(f"unknown {what} options {unknown}")
        o = struct()
        default(C.byref(o))
        kinds = dict(struct._fields_)
        for k, v in options.items():
            if names and k in names and isinstance(v, str):
                v = names[k][v]
            if issubclass(kinds[k], C.Array):
                getattr(o, k)[:] = [float(x) for x in v]
            else:
                setattr(o, k, float(v) if kinds[k] is C.c_float else int(v))
        return o

    @classmethod
    def sky_options(cls, options=None):
        """None, an _lib.ow_sky_options, or a dict of srgb and energy over ow_sky_options_default's values"""
        return cls._options(_lib.ow_sky_options, _lib.load().ow_sky_options_default, cls._SKY_OWN, options, "sky")

    @classmethod
    def environment_options(cls, options=None):
        """None, an _lib.ow_environment_options, or a dict over ow_environment_options_default's values (the reference scene's depth fog) that may
        set fog_mode ("depth" / "exponential" or the number), density, depth_begin, depth_end, depth_curve, aerial_perspective, sun_scatter,
        light_color, sun_color, sun_direction and sky_color"""
        return cls._options(_lib.ow_environment_options, _lib.load().ow_environment_options_default, cls._ENVIRONMENT_OWN, options, "environment",
                            {"fog_mode": cls.FOG_MODES})

    @classmethod
    def present_options(cls, options=None):
        """None, an _lib.ow_present_options, or a dict over ow_present_options_default's values (filmic, sRGB, the scene's adjustments) that may
        set downsample, tonemap ("linear" / "reinhard" / "filmic" or the number), exposure, white, srgb, brightness, contrast and saturation"""
        return cls._options(_lib.ow_present_options, _lib.load().ow_present_options_default, cls._PRESENT_OWN, options, "present",
                            {"tonemap": cls.TONEMAPS})

    def sky_create(self, panorama_rgba8, options=None):
        """A panorama from an (H, W, 4) uint8 equirectangular image, rows from the top, uploaded once; returns a Sky (sky_destroy() it before
        free())"""
        img = np.ascontiguousarray(panorama_rgba8, np.uint8)
        if img.ndim != 3 or img.shape[2] != 4:
            raise ValueError("a panorama is (height, width, 4) uint8")
        o = self.sky_options(options)
        out = C.c_void_p()
        _lib.check(self._lib.ow_sky_create(self.context, _ref(o), img.ctypes.data, img.shape[1], img.shape[0], C.byref(out)))
        return Sky(out, img.shape[1], img.shape[0])

    def sky_destroy(self, sky):
        self._destroy(sky, self._lib.ow_sky_destroy)

    def environment_apply(self, camera, pixels, sky=None, options=None):
        """Sky fill and fog over `pixels` ((H, W) RENDER_PIXEL records of the draws): the records with color and status rewritten (a copy).
        Synchronises."""
        o = self.environment_options(options)
        _, rec = self._picture(camera, pixels, False)
        _lib.check(self._lib.ow_environment_apply(self.context, sky.handle if sky is not None else None, C.byref(camera), _ref(o), rec.ctypes.data))
        return rec

    def environment_apply_async(self, camera, pixels_device, sky=None, options=None):
        """The pass over DEVICE records (mesh_draw_async's), in place, enqueued in the generator's stream order without synchronising"""
        self._check_picture_buffers(camera, None, pixels_device)
        o = self.environment_options(options)
        _lib.check(self._lib.ow_environment_apply_async(self.context, sky.handle if sky is not None else None, C.byref(camera), _ref(o),
                                                        _addr(pixels_device)))

    @classmethod
    def present_size(cls, camera, options=None):
        """(height, width) of what present() returns for records of the camera's size"""
        o = cls.present_options(options)
        s = max(int(o.downsample), 1) if o is not None else 1
        return int(camera.height) // s, int(camera.width) // s

    def present(self, camera, pixels, options=None, linear=False):
        """The finished picture of `pixels` ((H, W) RENDER_PIXEL records; camera.width x camera.height is THEIR size): (H / s, W / s, 4) uint8 sRGB
        RGBA, or with linear=True the pair (RGBA, (H / s, W / s, 4) float32 resolved linear RGB and hit share).  Synchronises."""
        o = self.present_options(options)
        _, rec = self._picture(camera, pixels, False)
        h, w = self.present_size(camera, o)
        rgba = np.zeros((max(h, 1), max(w, 1), 4), np.uint8)
        lin = np.zeros((max(h, 1), max(w, 1), 4), np.float32) if linear else None
        _lib.check(self._lib.ow_present(self.context, C.byref(camera), _ref(o), rec.ctypes.data, rgba.ctypes.data,
                                        lin.ctypes.data if linear else None))
        return (rgba, lin) if linear else rgba

    def present_async(self, camera, pixels_device, rgba_device, linear_device=None, options=None):
        """The present over DEVICE buffers, enqueued in the generator's stream order without synchronising: pixels_device holds the camera's
        H * W records, rgba_device (H / s) * (W / s) * 4 bytes, linear_device as many float4; either output may be None (not both)"""
        o = self.present_options(options)
        h, w = self.present_size(camera, o)
        _check_device_size(pixels_device, int(camera.width) * int(camera.height), self.RENDER_PIXEL.itemsize, "pixels_device", "records")
        _check_device_size(rgba_device, h * w, 4, "rgba_device", "pixels")
        _check_device_size(linear_device, h * w, 16, "linear_device", "pixels")
        _lib.check(self._lib.ow_present_async(self.context, C.byref(camera), _ref(o), _addr(pixels_device), _addr(rgba_device, True),
                                              _addr(linear_device, True)))

    _RADIANCE_OWN = ("levels", "samples", "base_width")
    _SKY_LIGHT_OWN = ("ambient_energy", "reflection_energy", "specular")

    @classmethod
    def radiance_options(cls, options=None):
        """None, an _lib.ow_radiance_options, or a dict of levels, samples and base_width over ow_radiance_options_default's values"""
        return cls._options(_lib.ow_radiance_options, _lib.load().ow_radiance_options_default, cls._RADIANCE_OWN, options, "radiance")

    @classmethod
    def sky_light_options(cls, options=None):
        """None, an _lib.ow_radiance_light_options, or a dict of ambient_energy, reflection_energy and specular over
        ow_radiance_light_options_default's values (1, 1, 0.5)"""
        return cls._options(_lib.ow_radiance_light_options, _lib.load().ow_radiance_light_options_default, cls._SKY_LIGHT_OWN, options, "sky light")

    def radiance_create(self, sky, options=None):
        """The roughness-blurred pyramid and the irradiance of a Sky, built once on the device; returns a Radiance (radiance_destroy() it
        before free()).  The sky may be destroyed afterwards."""
        o = self.radiance_options(options)
        out, n = C.c_void_p(), C.c_int32()
        _lib.check(self._lib.ow_radiance_create(self.context, sky.handle, _ref(o), C.byref(out)))
        _lib.check(self._lib.ow_radiance_level(self.context, out, 0, C.byref(n), None, None, None))
        return Radiance(out, n.value)

    def radiance_destroy(self, radiance):
        self._destroy(radiance, self._lib.ow_radiance_destroy)

    def radiance_level(self, radiance, level):
        """(H, W, 4) float32 texels of level `level` (0 .. levels - 1), or of the 16 x 32 irradiance with level="irradiance".  Synchronises."""
        k = _lib.OW_RADIANCE_IRRADIANCE if level == "irradiance" else int(level)
        w, h = C.c_int32(), C.c_int32()
        _lib.check(self._lib.ow_radiance_level(self.context, radiance.handle, k, None, C.byref(w), C.byref(h), None))
        out = np.zeros((h.value, w.value, 4), np.float32)
        _lib.check(self._lib.ow_radiance_level(self.context, radiance.handle, k, None, None, None, out.ctypes.data))
        return out

    def sky_light_apply(self, radiance, camera, pixels, options=None):
        """Sky ambient and sky reflection over `pixels` ((H, W) RENDER_PIXEL records of the draws, made with ambient_color 0): the records
        with color and status rewritten (a copy).  Call it before environment_apply.  Synchronises."""
        o = self.sky_light_options(options)
        _, rec = self._picture(camera, pixels, False)
        _lib.check(self._lib.ow_radiance_light_apply(self.context, radiance.handle if radiance is not None else None, C.byref(camera), _ref(o),
                                                     rec.ctypes.data))
        return rec

    def sky_light_apply_async(self, radiance, camera, pixels_device, options=None):
        """The pass over DEVICE records (mesh_draw_async's), in place, enqueued in the generator's stream order without synchronising"""
        self._check_picture_buffers(camera, None, pixels_device)
        o = self.sky_light_options(options)
        _lib.check(self._lib.ow_radiance_light_apply_async(self.context, radiance.handle if radiance is not None else None, C.byref(camera), _ref(o),
                                                           _addr(pixels_device)))

    # ---- the floating bodies' sun shadows (include/ocean_waves.h ow_shadow_*) ----
    _SHADOW_FRAME_OWN = ("light_direction", "half_extent", "center", "depth_range", "cast_both_sides", "lane_box")
    _SHADOW_OWN = ("bias", "normal_bias", "opacity", "filter_taps", "receive_water")

    @classmethod
    def shadow_frame(cls, frame=None):
        """an _lib.ow_shadow_frame, or None / a dict of light_direction, half_extent, center, depth_range, cast_both_sides and lane_box over
        ow_shadow_frame_default's values (the scene's sun, 100 m about the origin, 100 m either side along the light)"""
        if isinstance(frame, _lib.ow_shadow_frame):
            return frame
        frame = dict(frame or {})
        flags = _lib.OW_SHADOW_CAST_BOTH_SIDES if frame.pop("cast_both_sides", False) else 0
        o = cls._options(_lib.ow_shadow_frame, _lib.load().ow_shadow_frame_default, cls._SHADOW_FRAME_OWN, frame, "shadow frame")
        o.flags |= flags
        return o

    @classmethod
    def shadow_options(cls, options=None):
        """None, an _lib.ow_shadow_options, or a dict of bias, normal_bias, opacity, filter_taps and receive_water over
        ow_shadow_options_default's values (0, 6.464, 0.8, 5 taps, water does not receive)"""
        if options is None or isinstance(options, _lib.ow_shadow_options):
            return options
        options = dict(options)
        flags = _lib.OW_SHADOW_RECEIVE_WATER if options.pop("receive_water", False) else 0
        o = cls._options(_lib.ow_shadow_options, _lib.load().ow_shadow_options_default, cls._SHADOW_OWN, options, "shadow")
        o.flags |= flags
        return o

    def shadow_map_create(self, size):
        """An empty size x size depth map from the sun, without a frame; returns a ShadowMap (shadow_map_destroy() it before free())"""
        out = C.c_void_p()
        _lib.check(self._lib.ow_shadow_map_create(self.context, int(size), C.byref(out)))
        return ShadowMap(out, int(size))

    def shadow_map_destroy(self, shadow_map):
        self._destroy(shadow_map, self._lib.ow_shadow_map_destroy)

    def shadow_map_begin(self, shadow_map, frame=None):
        """Sets the frame and clears the map and its counters, enqueued in the generator's stream order without synchronising"""
        _lib.check(self._lib.ow_shadow_map_begin(self.context, shadow_map.handle, C.byref(self.shadow_frame(frame))))

    def shadow_map_cast(self, shadow_map, solid, bodies_set, first=0, count=None):
        """Casts the shape at the resident poses of bodies [first, first + count) into the map, enqueued without synchronising"""
        count = bodies_set.num_bodies - first if count is None else count
        _lib.check(self._lib.ow_shadow_map_cast(self.context, shadow_map.handle, solid.handle, bodies_set.handle, int(first), int(count)))

    def shadow_map_cast_instances(self, shadow_map, solid, transforms):
        """shadow_map_cast over a host array of [count][12] transforms (basis rows, then the origin).  Synchronises."""
        t = np.ascontiguousarray(transforms, np.float32).reshape(-1, 12)
        _lib.check(self._lib.ow_shadow_map_cast_instances(self.context, shadow_map.handle, solid.handle, t.ctypes.data if len(t) else None, len(t)))

    def shadow_map_read(self, shadow_map):
        """(size, size) float32 depths in metres from the frame's near plane, FLT_MAX where nothing was cast.  Synchronises."""
        out = np.zeros((shadow_map.size, shadow_map.size), np.float32)
        _lib.check(self._lib.ow_shadow_map_read(self.context, shadow_map.handle, out.ctypes.data))
        return out

    def shadow_apply(self, shadow_map, camera, pixels, options=None, rgba=False):
        """The sun's share of `pixels` ((H, W) RENDER_PIXEL records of the draws) darkened by the map: (the (H, W, 4) uint8 RGBA image or
        None, the records with status, diffuse, specular and color rewritten (a copy)).  Call it after solid_draw and before
        sky_light_apply and environment_apply.  Synchronises."""
        o = self.shadow_options(options)
        img, rec = self._picture(camera, pixels, rgba)
        _lib.check(self._lib.ow_shadow_apply(self.context, shadow_map.handle if shadow_map is not None else None, C.byref(camera), _ref(o),
                                             rec.ctypes.data, img.ctypes.data if img is not None else None))
        return img, rec

    def shadow_apply_async(self, shadow_map, camera, pixels_device, rgba_device=None, options=None):
        """The pass over DEVICE records (mesh_draw_async's), in place, enqueued in the generator's stream order without synchronising"""
        self._check_picture_buffers(camera, rgba_device, pixels_device)
        o = self.shadow_options(options)
        _lib.check(self._lib.ow_shadow_apply_async(self.context, shadow_map.handle if shadow_map is not None else None, C.byref(camera), _ref(o),
                                                   _addr(pixels_device), _addr(rgba_device, True)))

    def shadow_stats(self, shadow_map, counters=True):
        """dict of the casts since the map's last begin, the scratch bytes held and, with counters (synchronising), the instances skipped and
        the triangles culled and drawn"""
        v = [C.c_uint64() for _ in range(5)]
        _lib.check(self._lib.ow_shadow_stats(self.context, shadow_map.handle, C.byref(v[0]), *(C.byref(x) if counters else None for x in v[1:4]),
                                             C.byref(v[4])))
        keys = ("casts", "skipped_instances", "culled", "drawn", "scratch_bytes")
        return {k: x.value for k, x in zip(keys, v) if counters or k in ("casts", "scratch_bytes")}

    def get_push_constants(self, cascade):
        """(spectrum[16], modulate[8], unpack[4]) uint32 words: the reference's push-constant blocks of this cascade's most recent launch"""
        pc = _lib.ow_push_constants()
        _lib.check(self._lib.ow_get_push_constants(self.context, cascade, C.byref(pc)))
        return (np.array(pc.spectrum, np.uint32), np.array(pc.modulate, np.uint32), np.array(pc.unpack, np.uint32))

    def get_maps_f32(self, cascade):
        out = np.empty((self.map_size, self.map_size, 8), np.float32)
        _lib.check(self._lib.ow_get_maps_f32(self.context, cascade, out.ctypes.data))
        return out

    def get_spectrum(self, cascade):
        n = self.map_size
        h0, om = np.empty((n, n, 4), np.float32), np.empty((n, n), np.float32)
        _lib.check(self._lib.ow_get_spectrum(self.context, cascade, h0.ctypes.data, om.ctypes.data))
        return h0, om

    def debug_set_spectrum(self, cascade, h0, omega=None):
        """test hook (ow_debug_set_spectrum): h0 complex64 [n][n] = h0(k) as [y][x] replaces the resident spectrum of `cascade`; omega float32
        [n][n] replaces its dispersion plane (None keeps it)"""
        n = self.map_size
        h0 = np.ascontiguousarray(h0, np.complex64)
        if h0.shape != (n, n):
            raise ValueError(f"h0 must be [{n}][{n}], got {h0.shape}")
        if omega is not None:
            omega = np.ascontiguousarray(omega, np.float32)
            if omega.shape != (n, n):
                raise ValueError(f"omega must be [{n}][{n}], got {omega.shape}")
        _lib.check(self._lib.ow_debug_set_spectrum(self.context, cascade, h0.ctypes.data, omega.ctypes.data if omega is not None else None))

    def get_intermediate(self, cascade):
        out = np.empty((4, self.map_size, self.map_size, 2), np.float32)
        _lib.check(self._lib.ow_get_intermediate(self.context, cascade, out.ctypes.data))
        return out

    KERNEL_FAMILIES = {0: None, 1: "standard", 2: "layer_parallel", 3: "compact", 4: "layer_parallel_compact", 5: "tick_groups_compact",
                       6: "tick_pairs_compact"}

    def last_kernel_family(self):
        """which kernels the most recent batch ran with: "standard", "layer_parallel", "compact" (None before the first launch)"""
        return self.KERNEL_FAMILIES[int(self._lib.ow_last_kernel_family(self.context))]

    def last_batch_cascades(self):
        """cascades in the most recent pair of launches (a tick may be split into several pairs)"""
        return int(self._lib.ow_last_batch_cascades(self.context))

    def tick_group_depth(self):
        """ticks per launch: of the most recent run() that went out in tick groups / tick pairs, else the depth planned for this
        context's small batches (0: no tick groups)"""
        return int(self._lib.ow_tick_group_depth(self.context))

    def lookahead_stats(self):
        """(hits, speculated): update_all() ticks whose pass 1 had been speculated by the previous call, and speculations launched"""
        h, sp = C.c_uint64(), C.c_uint64()
        _lib.check(self._lib.ow_lookahead_stats(self.context, C.byref(h), C.byref(sp)))
        return h.value, sp.value

    def chain_stats(self):
        """launches that went out as two chains on two streams (1024^2, four cascades a side; OW_FLAG_SINGLE_STREAM keeps them whole)"""
        n = C.c_uint64()
        _lib.check(self._lib.ow_chain_stats(self.context, C.byref(n)))
        return n.value

    def spectrum_stats(self):
        """(generated, skipped): spectrum kernels launched, and dirty flags consumed because the resident spectrum had been generated from the
        same thirteen packed constants (a whitecap / foam_amount edit: wave_cascade_parameters.gd:32-35 raise the flag, spectrum_compute never reads them)"""
        g, sk = C.c_uint64(), C.c_uint64()
        _lib.check(self._lib.ow_spectrum_stats(self.context, C.byref(g), C.byref(sk)))
        return g.value, sk.value

    def timing(self, enable):
        """False / 0: off; True / 1: per pass (run() stays on one launch per pass); 2: as launched (tick groups / pairs stay on and are
        timed per launch: timing_read_launches)"""
        _lib.check(self._lib.ow_timing_enable(self.context, 2 if enable == 2 else (1 if enable else 0)))

    def probe_kernel_times(self, reps=50):
        """(pass1_ms, pass2_ms, cascades_per_launch): each kernel alone, `reps` back-to-back launches (benchmark probe;
        the extra pass-2 launches advance the foam state)"""
        a, b, n = C.c_float(), C.c_float(), C.c_int32()
        _lib.check(self._lib.ow_probe_kernel_times(self.context, reps, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def timing_read_launches(self, reset=True):
        """(average ms, count) of the tick-group / tick-pair launches timed under timing(2)"""
        a, n = C.c_float(), C.c_int32()
        _lib.check(self._lib.ow_timing_read_launches(self.context, C.byref(a), C.byref(n), 1 if reset else 0))
        return a.value, n.value

    def timing_read(self, reset=True):
        a, b, n = C.c_float(), C.c_float(), C.c_int32()
        _lib.check(self._lib.ow_timing_read(self.context, C.byref(a), C.byref(b), C.byref(n), 1 if reset else 0))
        return a.value, b.value, n.value

"""What the wrapper's subsystem modules share: the argument helpers, the handle classes, the seventeen record dtypes, the one dict-to-struct
converter and the host arrays of a picture call.  No entry point of its own: the modules beside it (_points, _bodies, _mesh, _spray, _solid,
_sky, _lab, one per ow_*_host.hip unit) hold the calls, wave_generator.py assembles them into WaveGenerator.
"""
import ctypes as C

import numpy as np

from . import _lib


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


def _data(a):
    """an optional host array argument: NULL for None"""
    return a.ctypes.data if a is not None else None


def _handle(obj):
    """an optional handle object's handle: NULL for None"""
    return obj.handle if obj is not None else None


def _check_device_size(buf, count, size, name="out_device", unit="records"):
    """ValueError for a device buffer that knows its size and holds fewer than `count` units of `size` bytes; a bare address passes"""
    if hasattr(buf, "numel") and hasattr(buf, "element_size") and buf.numel() * buf.element_size() < count * size:
        raise ValueError(f"{name} holds fewer than {count} {unit} of {size} bytes")


def _count(given, buf, per_record, name="count"):
    """how many records an _async call works on: as given, else the tensor's size over per_record (elements with an int, bytes with the
    record's dtype); ValueError for a raw address, which does not know its size"""
    if given is not None:
        return int(given)
    if not hasattr(buf, "numel"):
        raise ValueError(f"{name} is needed for a raw device address")
    if isinstance(per_record, int):
        return int(buf.numel()) // per_record
    return int(buf.numel() * buf.element_size()) // per_record.itemsize


def _rest(bodies_set, first, count):
    """the count of bodies [first, first + count): None is up to the set's last one"""
    return bodies_set.num_bodies - first if count is None else count


def _stats(fn, handles, keys, skip=(), kinds=None):
    """a stats call: one out-parameter per key after the handles (uint64 unless `kinds` names another, NULL for the keys in `skip`, whose
    counters would synchronise); the dict of the keys that were asked for"""
    v = {k: (kinds or {}).get(k, C.c_uint64)() for k in keys}
    _lib.check(fn(*handles, *[None if k in skip else C.byref(x) for k, x in v.items()]))
    return {k: x.value for k, x in v.items() if k not in skip}


def _create_shape(fn, context, vertices, triangles):
    """what mesh_create and solid_create do: [V][3] float32 positions and [T][3] int32 indices to the device; (handle, V, T)"""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    out = C.c_void_p()
    _lib.check(fn(context, v.ctypes.data, len(v), t.ctypes.data, len(t), C.byref(out)))
    return out, len(v), len(t)


def _fill(o, values, names=None):
    """a dict's values into the struct's fields of the same names: arrays from sequences of floats, FP fields through float(), the others
    through int().  names: key -> {word: value} for an enumeration given as a word, or a function that reads the value first"""
    kinds = dict(o._fields_)
    for k, v in values.items():
        if k not in kinds:          # an allowed key that is no field (a flag, a falloff centre) is its converter's own business
            continue
        if names and k in names:
            v = names[k](v) if callable(names[k]) else names[k][v] if isinstance(v, str) else v
        if issubclass(kinds[k], C.Array):
            getattr(o, k)[:] = [float(x) for x in v]
        else:
            setattr(o, k, float(v) if kinds[k] in (C.c_float, C.c_double) else int(v))


def _camera_xz(camera):
    """the centre of "falloff": True without a falloff_center: the camera's x and z"""
    if camera is None:
        raise ValueError("falloff without a falloff_center needs the camera")
    return camera.position[0], camera.position[2]


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


class Shared:
    """the part of WaveGenerator every subsystem leans on.  The record dtypes are numpy's reading of the _lib structures, which test_abi holds
    to include/ocean_waves.h: a layout is declared there and in _lib.py, nowhere else."""
    SURFACE_SAMPLE = np.dtype(_lib.ow_surface_sample)
    SURFACE_QUERY = np.dtype(_lib.ow_surface_query)
    SURFACE_VELOCITY = np.dtype(_lib.ow_surface_velocity)
    BUOYANCY_BODY = np.dtype(_lib.ow_buoyancy_body)
    HULL_POINT = np.dtype(_lib.ow_hull_point)
    BUOYANCY_OPTIONS = np.dtype(_lib.ow_buoyancy_options)
    BUOYANCY_POINT = np.dtype(_lib.ow_buoyancy_point)
    BUOYANCY_RESULT = np.dtype(_lib.ow_buoyancy_result)
    RIGID_BODY = np.dtype(_lib.ow_rigid_body)
    BODIES_OPTIONS = np.dtype(_lib.ow_bodies_options)
    RAY = np.dtype(_lib.ow_ray)
    RAYCAST_OPTIONS = np.dtype(_lib.ow_raycast_options)
    RAYCAST_HIT = np.dtype(_lib.ow_raycast_hit)
    RENDER_PIXEL = np.dtype(_lib.ow_render_pixel)
    MESH_VERTEX = np.dtype(_lib.ow_mesh_vertex)
    SPRAY_INSTANCE = np.dtype(_lib.ow_spray_instance)
    SPRAY_PARTICLE = np.dtype(_lib.ow_spray_particle)

    @staticmethod
    def _options(struct, default, own, options, what, names=None):
        """The one dict-to-struct converter.  None or a struct pass; a dict is laid over the default's values (default None: over zeros)
        after a ValueError for a key outside `own`, which names them in the dict's order.  A key in `own` that is no field of the struct is
        left to the caller; names: see _fill"""
        if options is None or isinstance(options, struct):
            return options
        unknown = [k for k in options if k not in own]
        if unknown:
            raise ValueError(f"unknown {what} options {unknown}")
        o = struct()
        if default is not None:
            default(C.byref(o))
        _fill(o, options, names)
        return o

    def _destroy(self, obj, fn):
        """what every *_destroy does: the handle object is spent afterwards, a second destroy of it does nothing"""
        if obj.handle:
            fn(self.context, obj.handle)
            obj.handle = None

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
